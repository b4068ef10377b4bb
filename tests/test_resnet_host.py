"""The ResNet backbone without a GPU: the fp64 restatement (resnet_cases.py) against plain torch with the roundings off and the norm
unfolded, the fp32 fold recipe against the fp64 fold, sbev_resnet_plan as a literal table with its refusals, the C entries' argument
validation (which returns before any HIP call), torchvision's / mmdet's state-dict names, and ResNetBackbone's own refusals."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import resnet_cases as RC
from sparsebev_amd import _lib
from sparsebev_amd import resnet
from sparsebev_amd._lib import SbevError

EPS32 = float(torch.tensor(RC.EPS, dtype=torch.float32))          # the fp32 number the device adds to the variance


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def bn(x, params, name):
    return F.batch_norm(x, params[name + '.running_mean'].double(), params[name + '.running_var'].double(), params[name + '.weight'].double(),
                        params[name + '.bias'].double(), False, 0.0, EPS32)


def close(got, want):
    # two orders of summing the same fp64 products, and a scale applied before or after the sum: a few ulps of the largest partial sum
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert (got - want).abs().max() <= 1e-12 * max(1.0, float(want.abs().max()))


def test_restatement_of_stem_pool_and_bottlenecks_equals_plain_torch_in_fp64():
    """one stride-1 and one stride-2 Bottleneck with downsample behind the stem and the pool, on a 9 x 13 image (odd at every step)"""
    blocks = (1, 1)
    params = RC.real_params(blocks, seed=2)
    x = torch.randn(2, 3, 9, 13, generator=torch.Generator().manual_seed(3))
    acts = RC.reference(x, params, blocks, rounded=False)
    P = {k: v.double() for k, v in params.items()}
    y = F.relu(bn(F.conv2d(x.double(), P['conv1.weight'], stride=2, padding=3), params, 'bn1'))
    close(acts[0], y)
    assert torch.equal(RC.max_pool(y), F.max_pool2d(y, 3, 2, 1))          # a true maximum: exact on the same input
    y = F.max_pool2d(y, 3, 2, 1)
    close(acts[1], y)
    assert tuple(y.shape[2:]) == (3, 4)
    at = 2
    for s in range(2):
        pre, st = 'layer%d.0.' % (s + 1), 1 + s
        t = F.relu(bn(F.conv2d(y, P[pre + 'conv1.weight']), params, pre + 'bn1'))
        close(acts[at], t)
        t = F.relu(bn(F.conv2d(t, P[pre + 'conv2.weight'], stride=st, padding=1), params, pre + 'bn2'))
        close(acts[at + 1], t)
        idt = bn(F.conv2d(y, P[pre + 'downsample.0.weight'], stride=st), params, pre + 'downsample.1')
        close(acts[at + 2], idt)
        y = F.relu(bn(F.conv2d(t, P[pre + 'conv3.weight']), params, pre + 'bn3') + idt)
        close(acts[at + 3], y)
        at += 4
    assert at == len(acts) and tuple(y.shape) == (2, 512, 2, 2)
    # and with the roundings on every activation holds fp16 values
    rounded = RC.reference(x, params, blocks)
    assert all(torch.equal(a, a.half().double()) for a in rounded) and not torch.equal(rounded[0], acts[0])


def test_fp32_fold_recipe_is_within_one_ulp_of_the_fp64_fold():
    """s = gamma / sqrt(var + eps) in three individually rounded fp32 operations against fp64: within 1 ulp of fp32, read as the relative
    unit 2^-23 |s| (fp32's spacing at the top of a binade).  With u = 2^-24 per rounding the recipe's worst case is 2.5 u = 1.25 x 2^-23
    (the square root halves the sum's error), so the bound is no theorem; on these 4096 channels the largest error is 0.93 x 2^-23.
    Measured in the spacing at s itself (half as wide at the bottom of a binade) the same errors reach 1.46 spacings, on 43 channels:
    that reading cannot hold for any three-rounding recipe.  w s carries one rounding more, 3.5 u |w s| < 4 spacings; b' = beta - mean s
    carries 3.5 u |mean s| + u |b'| <= 5.5 u max(|beta|, |mean s|) < 6 spacings at that magnitude (b' cancels: its own is no yardstick)."""
    g = torch.Generator().manual_seed(7)
    co = 4096
    w = torch.randn(co, 8, 1, 1, generator=g)
    gamma, beta, mean = 0.5 + torch.rand(co, generator=g), torch.randn(co, generator=g), torch.randn(co, generator=g)
    var = 0.01 + 4 * torch.rand(co, generator=g)
    s32 = RC.scale32(gamma, var)
    wq, bq = RC.fold32(w, gamma, beta, mean, var)
    s64, w64, b64 = RC.fold64(w, gamma, beta, mean, var)
    ulp = lambda t: 2.0 ** (torch.floor(torch.log2(t.abs().double().clamp_min(2.0 ** -126))) - 23)
    assert ((s32.double() - s64).abs() <= 2.0 ** -23 * s64.abs()).all()
    p32 = w * s32[:, None, None, None]
    assert ((p32.double() - w64).abs() <= 4 * ulp(w64)).all()
    assert torch.equal(wq, p32.half()) and wq.dtype == torch.float16 and bq.dtype == torch.float32
    big = torch.maximum(beta.abs(), (mean * s32).abs())
    assert ((bq.double() - b64).abs() <= 6 * ulp(big)).all()
    # the integer norm of the exact tests folds to integers
    gi, bi, mi, vi = RC.integer_norm(256, g)
    assert torch.equal(vi + torch.tensor(RC.EPS, dtype=torch.float32), torch.ones(256))
    wq, bq = RC.fold32(torch.ones(256, 1, 1, 1), gi, bi, mi, vi)
    assert torch.equal(wq.float().view(-1), gi) and torch.equal(bq, bi - mi * gi) and torch.equal(bq, bq.round())


def conv_row(cin, cout, taps, stride, h, w, row_tiles, col_tiles, epilogue, k_split=1):
    return dict(kind='conv', cin=cin, cout=cout, taps=taps, stride=stride, h=h, w=w, row_tiles=row_tiles, col_tiles=col_tiles, k_split=k_split,
                epilogue=epilogue)


def test_plan_literal_table_r50_6x256x704():
    p = resnet.plan(50, 6, 256, 704)
    assert p['launches'] == 54 and len(p['layers']) == 54
    assert p['outs'] == [(256, 64, 176), (512, 32, 88), (1024, 16, 44), (2048, 8, 22)]
    strip = lambda d: {k: v for k, v in d.items() if k != 'where'}
    L = p['layers']
    assert strip(L[0]) == dict(kind='stem', cin=3, cout=64, taps=49, stride=2, h=128, w=352, row_tiles=2112, col_tiles=1, k_split=1, epilogue=1)
    assert strip(L[1]) == dict(kind='pool', cin=64, cout=64, taps=9, stride=2, h=64, w=176, row_tiles=528, col_tiles=1, k_split=1, epilogue=0)
    # stage 1, block 0: conv1, conv2, downsample, conv3 (67 584 rows: 528 tiles; 256 channels in one column tile)
    assert [strip(l) for l in L[2:6]] == [conv_row(64, 64, 1, 1, 64, 176, 528, 1, 1), conv_row(64, 64, 9, 1, 64, 176, 528, 1, 1),
                                          conv_row(64, 256, 1, 1, 64, 176, 528, 1, 0), conv_row(64, 256, 1, 1, 64, 176, 528, 1, 2)]
    assert strip(L[6]) == conv_row(256, 64, 1, 1, 64, 176, 528, 1, 1)
    # stage 2, block 0 (16 896 rows: 132 tiles): 128 channels in two tiles of 64, 512 in two of 256
    assert [strip(l) for l in L[12:16]] == [conv_row(256, 128, 1, 1, 64, 176, 528, 1, 1), conv_row(128, 128, 9, 2, 32, 88, 132, 2, 1),
                                            conv_row(256, 512, 1, 2, 32, 88, 132, 2, 0), conv_row(128, 512, 1, 1, 32, 88, 132, 2, 2)]
    # stage 3, block 0 (4 224 rows: 33 tiles): 256 channels in four tiles of 64 (two of 128 on the 132-tile input plane), 1024 in eight of 128
    assert [strip(l) for l in L[25:29]] == [conv_row(512, 256, 1, 1, 32, 88, 132, 2, 1), conv_row(256, 256, 9, 2, 16, 44, 33, 4, 1, k_split=3),
                                            conv_row(512, 1024, 1, 2, 16, 44, 33, 8, 0), conv_row(256, 1024, 1, 1, 16, 44, 33, 8, 2)]
    assert strip(L[29]) == conv_row(1024, 256, 1, 1, 16, 44, 33, 4, 1, k_split=3)
    # stage 4, block 0 (1 056 rows: 9 tiles): tiles of 64 channels everywhere; fewer than 256 workgroups of them and 6 chunks or more: K split in 3
    assert [strip(l) for l in L[44:48]] == [conv_row(1024, 512, 1, 1, 16, 44, 33, 8, 1), conv_row(512, 512, 9, 2, 8, 22, 9, 8, 1, k_split=3),
                                            conv_row(1024, 2048, 1, 2, 8, 22, 9, 32, 0), conv_row(512, 2048, 1, 1, 8, 22, 9, 32, 2)]
    assert strip(L[53]) == conv_row(512, 2048, 1, 1, 8, 22, 9, 32, 2)
    assert [i for i, l in enumerate(L) if l['k_split'] == 3] == [26, 29, 30, 32, 33, 35, 36, 38, 39, 41, 42, 45, 48, 49, 51, 52]
    # the stage outputs live in the caller's tensors, everything else in five reused regions of the workspace
    ends = RC.stage_ends((3, 4, 6, 3))
    assert [L[e]['where'] for e in ends] == [-1, -2, -3, -4]
    assert all(l['where'] >= 0 for i, l in enumerate(L) if i not in ends) and len({l['where'] for l in L}) == 4 + 5
    # the architecture's numbers: weights (fp16) + biases (fp32), multiply-adds
    convs = [l for l in RC.net_layers((3, 4, 6, 3)) if l['kind'] != 'pool']
    pack = sum((160 if l['k'] == 7 else l['k'] ** 2 * l['cin']) * l['cout'] * 2 + 4 * l['cout'] for l in convs)
    assert p['pack_bytes'] == pack
    macs = sum(6 * r['h'] * r['w'] * r['cout'] * (147 if r['kind'] == 'stem' else r['taps'] * r['cin']) for r in L if r['kind'] != 'pool')
    assert p['macs'] == macs and 14.0e9 < macs / 6 < 15.5e9
    act = lambda rows, c: (rows * c * 2 + 255) // 256 * 256
    assert p['workspace_bytes'] == 2 * act(67584, 256) + act(6 * 128 * 352, 64) + act(67584, 64) + act(67584, 256)
    # keep: one region per launch
    k = resnet.plan(50, 6, 256, 704, keep=True)
    assert len({l['where'] for l in k['layers']}) == 54 and k['workspace_bytes'] > p['workspace_bytes']
    # depth 101, other out_indices, no images, the smallest image
    assert resnet.plan(101, 1, 256, 704)['launches'] == 2 + 3 * 33 + 4
    q = resnet.plan(50, 2, 40, 72, out_indices=(1, 3))
    assert q['outs'] == [(512, 5, 9), (2048, 2, 3)] and [l['where'] for l in q['layers'] if l['where'] < 0] == [-1, -2]
    assert [(l['h'], l['w']) for l in q['layers'][:3]] == [(20, 36), (10, 18), (10, 18)]
    z = resnet.plan(50, 0, 256, 704)
    assert z['launches'] == 0 and z['workspace_bytes'] == 0 and z['pack_bytes'] == pack
    assert resnet.plan(50, 1, 1, 1)['outs'] == [(256, 1, 1), (512, 1, 1), (1024, 1, 1), (2048, 1, 1)]


def test_plan_refusals():
    table = [
        (dict(base_channels=96), 'multiples of 64'),
        (dict(base_channels=32), 'multiples of 64'),
        (dict(depth=18), 'BasicBlock'),
        (dict(depth=34), 'BasicBlock'),
        (dict(depth=49), 'depth=49'),
        (dict(n=-1), 'n=-1'),
        (dict(H=0), 'empty image'),
        (dict(W=32768), 'a side above 32767'),
        (dict(n=4096, H=8192, W=8192), '32-bit row indices'),
        (dict(out_indices=(2, 1)), 'increasing'),
        (dict(out_indices=(4,)), 'increasing'),
        (dict(num_stages=5, out_indices=(0,)), 'num_stages=5'),
        (dict(stage_blocks=(3, 4, 60, 3)), 'more than 160 launches'),
    ]
    for overrides, text in table:
        args = dict(depth=50, n=1, H=64, W=64)
        args.update(overrides)
        with pytest.raises(SbevError, match=text):
            resnet.plan(**args)


def test_c_entries_validate_before_any_gpu_call(lib):
    one, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1008)
    err = lambda: lib.sbev_last_error().decode()
    conv = lambda x=one, pack=one, res=None, y=one, n=1, H=4, W=4, cin=64, cout=64, taps=1, stride=1, epi=0, ct=0: lib.sbev_conv_f16(
        x, pack, res, y, n, H, W, cin, cout, taps, stride, epi, ct, None)
    table = [
        (dict(taps=4), 'taps=4'), (dict(stride=3), 'stride=3'), (dict(epi=3), 'epilogue=3'), (dict(cin=96), '96 input channels'),
        (dict(cout=32), '32 output channels'), (dict(ct=128), 'col_tile=128'), (dict(ct=32), 'col_tile=32'), (dict(n=-1), 'n=-1'),
        (dict(H=0), 'empty plane'), (dict(W=40000), 'a side above 32767'), (dict(n=1 << 20, H=256, W=256), 'row indices are 32-bit'),
        (dict(x=None), 'null pointer'), (dict(pack=None), 'null pointer'), (dict(y=None), 'null pointer'), (dict(epi=2), 'null pointer'),
        (dict(x=odd), '16-byte alignment'), (dict(pack=odd), '16-byte alignment'), (dict(y=odd), '16-byte alignment'),
        (dict(epi=2, res=odd), '16-byte alignment'),
    ]
    for overrides, text in table:
        assert conv(**overrides) == -1 and text in err(), (overrides, err())
    assert conv(n=0, x=None, pack=None, y=None) == 0                      # an empty call answers before the pointers are looked at
    assert conv(n=0, cin=96) == -1

    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)
    ptrs = lambda *v: (ctypes.c_void_p * len(v))(*v)
    blocks, idx = i32(1, 1, 1, 1), i32(0, 1, 2, 3)
    outs = ptrs(0x1000, 0x1000, 0x1000, 0x1000)
    fwd = lambda depth=50, n=1, x=one, dt=0, pack=one, ws=one, outs=outs, H=32, base=64: lib.sbev_resnet_forward(
        depth, blocks, 4, base, n, H, 32, 4, idx, 0, x, dt, pack, ws, outs, None)
    for overrides, text in [(dict(depth=34), 'BasicBlock'), (dict(base=100), 'multiples of 64'), (dict(dt=1), 'x_dtype 1'), (dict(dt=3), 'x_dtype 3'),
                            (dict(x=None), 'null pointer'), (dict(pack=None), 'null pointer'), (dict(ws=None), 'null pointer'),
                            (dict(outs=None), 'null pointer'), (dict(outs=ptrs(0x1000, 0, 0x1000, 0x1000)), 'output 1: null pointer'),
                            (dict(x=odd), '16-byte alignment'), (dict(ws=odd), '16-byte alignment'),
                            (dict(outs=ptrs(0x1000, 0x1000, 0x1008, 0x1000)), '16-byte alignment'), (dict(H=0), 'empty image')]:
        assert fwd(**overrides) == -1 and text in err(), (overrides, err())
    assert fwd(n=0, x=None, pack=None, ws=None, outs=None) == 0

    w = ptrs(0x1000)
    pack = lambda n=1, desc=i32(64, 64, 1), w=w, g=w, eps=1e-5, dt=0, dst=one: lib.sbev_resnet_pack_weights(n, desc, w, g, w, w, w, eps, dt, dst, None)
    for overrides, text in [(dict(desc=i32(96, 64, 1)), '96 input channels'), (dict(desc=i32(64, 64, 49)), 'stem has 3 input channels'),
                            (dict(desc=i32(64, 64, 4)), 'taps=4'), (dict(dt=1), 'w_dtype 1'), (dict(n=161), '161 layers'), (dict(eps=-1.0), 'eps'),
                            (dict(w=None), 'null pointer'), (dict(dst=None), 'null pointer'), (dict(w=ptrs(0)), 'layer 0: null pointer'),
                            (dict(g=ptrs(0x1002)), 'misaligned'), (dict(dst=odd), '16-byte alignment')]:
        assert pack(**overrides) == -1 and text in err(), (overrides, err())
    assert pack(n=0, w=None, dst=None) == 0


@pytest.mark.parametrize('depth,count', [(50, 318), (101, 624)])
def test_state_dict_names_and_count(depth, count):
    from sparsebev_amd import ResNetBackbone
    net = ResNetBackbone(depth=depth)
    sd = net.state_dict()
    want = RC.state_dict_shapes(resnet.STAGE_BLOCKS[depth])
    assert len(sd) == count and {k: tuple(v.shape) for k, v in sd.items()} == want
    assert 'layer1.0.downsample.1.running_var' in sd and 'layer4.2.bn3.num_batches_tracked' in sd and 'layer1.1.downsample.0.weight' not in sd
    assert not any(p.requires_grad for p in net.parameters()) and not net.training
    assert [tuple(c.weight.shape) for c, _ in net.conv_bn_pairs()] == [s for k, s in want.items() if len(s) == 4]


def test_prefixed_checkpoint_loads_strict():
    from sparsebev_amd import ResNetBackbone
    blocks = (1, 2, 1, 1)
    params = RC.real_params(blocks, seed=4)
    ckpt = {'img_backbone.' + k: v for k, v in params.items()}
    ckpt['img_neck.lateral_convs.0.conv.weight'] = torch.zeros(1)
    net = ResNetBackbone(depth=50, stage_blocks=blocks)
    net.load_state_dict({k[len('img_backbone.'):]: v for k, v in ckpt.items() if k.startswith('img_backbone.')}, strict=True)
    assert torch.equal(net.layer2[1].bn3.running_var, params['layer2.1.bn3.running_var'])
    assert torch.equal(net.layer4[0].downsample[0].weight, params['layer4.0.downsample.0.weight'])
    with pytest.raises(RuntimeError):
        net.load_state_dict({k: v for k, v in params.items() if k != 'bn1.running_mean'}, strict=True)


def test_python_refusals():
    from sparsebev_amd import ResNetBackbone
    for kwargs, text in [(dict(style='caffe'), 'style'), (dict(depth=18), 'depth'), (dict(depth=34), 'depth'), (dict(dcn=dict(type='DCN')), 'dcn'),
                         (dict(deep_stem=True), 'deep_stem'), (dict(avg_down=True), 'avg_down'), (dict(dilations=(1, 1, 2, 4)), 'dilations'),
                         (dict(norm_eval=False), 'norm_eval'), (dict(out_dtype=torch.float32), 'out_dtype'), (dict(out_indices=(3, 4)), 'out_indices'),
                         (dict(base_channels=48), 'base_channels'), (dict(norm_cfg=dict(type='GN')), 'norm_cfg')]:
        with pytest.raises(ValueError, match=text):
            ResNetBackbone(**kwargs)
    # accepted without effect
    net = ResNetBackbone(depth=50, stage_blocks=(1, 1, 1, 1), frozen_stages=1, norm_eval=True, with_cp=True, zero_init_residual=False,
                         norm_cfg=dict(type='BN2d', requires_grad=True, eps=1e-3), init_cfg=None, pretrained=None)
    assert net.eps == 1e-3 and net.bn1.eps == 1e-3 and net.out_channels == [256, 512, 1024, 2048]
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match='device tensors'):
        net(x)
    with pytest.raises(ValueError, match=r'\[n, 3, H, W\]'):
        net(torch.zeros(1, 4, 8, 8))
    with pytest.raises(ValueError, match=r'\[n, 3, H, W\]'):
        net(torch.zeros(3, 8, 8))
