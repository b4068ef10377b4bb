"""The ResNet backbone's backward without a GPU: the fp64 restatement (resnet_bwd_cases.py) against torch.autograd in fp64 with the
roundings off (which proves the fold-backward identity for g_gamma), sbev_resnet_backward_plan as a literal table with its refusals, the
C entries' argument validation (which returns before any HIP call), ResNetBackbone(trainable=True)'s refusals and the parameters it
marks for training."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import resnet_bwd_cases as BC
import resnet_cases as RC
from sparsebev_amd import _lib
from sparsebev_amd import resnet
from sparsebev_amd._lib import SbevError

EPS32 = float(torch.tensor(RC.EPS, dtype=torch.float32))


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def torch_net(x, P, blocks):
    """Conv2d + eval BatchNorm2d + ReLU Bottlenecks in fp64 on leaf tensors P: the stage outputs"""
    bn = lambda t, name: F.batch_norm(t, P[name + '.running_mean'], P[name + '.running_var'], P[name + '.weight'], P[name + '.bias'], False, 0.0, EPS32)
    y = F.max_pool2d(F.relu(bn(F.conv2d(x, P['conv1.weight'], stride=2, padding=3), 'bn1')), 3, 2, 1)
    outs = []
    for s, nb in enumerate(blocks):
        for b in range(nb):
            pre, st = 'layer%d.%d.' % (s + 1, b), 2 if (b == 0 and s > 0) else 1
            t = F.relu(bn(F.conv2d(y, P[pre + 'conv1.weight']), pre + 'bn1'))
            t = F.relu(bn(F.conv2d(t, P[pre + 'conv2.weight'], stride=st, padding=1), pre + 'bn2'))
            idt = bn(F.conv2d(y, P[pre + 'downsample.0.weight'], stride=st), pre + 'downsample.1') if b == 0 else y
            y = F.relu(bn(F.conv2d(t, P[pre + 'conv3.weight']), pre + 'bn3') + idt)
        outs.append(y)
    return outs


@pytest.fixture(scope='module')
def host_net():
    """the issue's host case once: parameters, the fp64 activations of every launch, torch's stage outputs and output gradients"""
    blocks = BC.HOST_BLOCKS
    params = RC.real_params(blocks, seed=21)
    g = torch.Generator().manual_seed(22)
    x = torch.randn(*BC.HOST_IMAGE, generator=g)
    acts = RC.reference(x, params, blocks, rounded=False)
    P = {k: v.double().requires_grad_(v.dim() > 0 and 'running' not in k) for k, v in params.items() if v.dim() > 0}
    with torch.enable_grad():
        outs = torch_net(x.double(), P, blocks)
        gouts = {s: torch.randn(o.shape, generator=g, dtype=torch.float64) for s, o in enumerate(outs)}
        sum((o * gouts[s]).sum() for s, o in enumerate(outs)).backward()
    return blocks, params, acts, P, gouts


@pytest.mark.parametrize('frozen_stages', [0, 1])
def test_restatement_equals_torch_autograd_in_fp64(host_net, frozen_stages):
    blocks, params, acts, P, gouts = host_net
    grads, stored, e = BC.backward(acts, params, blocks, gouts, frozen_stages + 1, rounded=False)
    names = BC.trainable_names(blocks, frozen_stages + 1)
    assert e == 0 and sorted(grads) == sorted(names)
    assert not any(k.startswith('conv1') or k.startswith('bn1') or (frozen_stages == 1 and k.startswith('layer1')) for k in grads)
    for name in names:
        want = P[name].grad
        assert grads[name].shape == want.shape
        assert (grads[name] - want).abs().max() <= 1e-12 * float(want.abs().max()), name
    # a stage map that is not an output adds nothing: drop stage 1's gradient and torch agrees once its loss term is gone
    assert len(stored) == 3 * (sum(blocks) - (blocks[0] if frozen_stages else 0))


def test_restatement_without_an_intermediate_output(host_net):
    """out_indices = (0, 3): the stage 2 and 3 maps get no addend"""
    blocks, params, acts, _, gouts = host_net
    P = {k: v.double().requires_grad_('running' not in k) for k, v in params.items() if v.dim() > 0}
    g = torch.Generator().manual_seed(22)
    x = torch.randn(*BC.HOST_IMAGE, generator=g)
    with torch.enable_grad():          # conftest runs every test under no_grad
        outs = torch_net(x.double(), P, blocks)
        ((outs[0] * gouts[0]).sum() + (outs[3] * gouts[3]).sum()).backward()
    grads, _, _ = BC.backward(acts, params, blocks, {0: gouts[0], 3: gouts[3]}, 2, rounded=False)
    for name in BC.trainable_names(blocks, 2):
        assert (grads[name] - P[name].grad).abs().max() <= 1e-12 * float(P[name].grad.abs().max()), name


def test_rounded_restatement_scales_and_stores_fp16(host_net):
    blocks, params, _, _, gouts = host_net
    x = torch.randn(*BC.HOST_IMAGE, generator=torch.Generator().manual_seed(22))
    acts = RC.reference(x, params, blocks)
    small = {s: (g * 1e-3).half().double() for s, g in gouts.items()}
    grads, stored, e = BC.backward(acts, params, blocks, small, 2)
    amax = max(float(g.abs().max()) for g in small.values())
    assert 8 <= 2.0 ** e * amax < 16
    assert all(torch.equal(g, g.half().double()) for g in stored.values())
    exact, _, _ = BC.backward(acts, params, blocks, small, 2, rounded=False)
    # fp16 operands in the window: the rounded definition follows the exact one to a few 2^-11 of the largest gradient
    for name in ('layer4.0.conv2.weight', 'layer2.0.bn1.weight', 'layer3.1.bn3.bias'):
        assert (grads[name] - exact[name]).abs().max() <= 2e-2 * float(exact[name].abs().max()), name
    assert BC.scale_exponent(0.0) == 0 and BC.scale_exponent(float('inf')) == 0 and BC.scale_exponent(float('nan')) == 0
    assert BC.scale_exponent(8.0) == 0 and BC.scale_exponent(15.9) == 0 and BC.scale_exponent(16.0) == -1 and BC.scale_exponent(2.0 ** -140) == 126


def test_slab_rule():
    assert [BC.slab_rule(p) for p in (1, 511, 512, 513, 8192, 8193, 67584)] == [(1, 512), (1, 512), (1, 512), (2, 512), (16, 512), (11, 768), (16, 4352)]
    assert all(resnet.wgrad_slabs(p) == BC.slab_rule(p) for p in (1, 511, 512, 513, 1056, 8192, 8193, 67584, 540672))


def test_backward_plan_literal_table_r50_6x256x704():
    p = resnet.backward_plan(50, 6, 256, 704, first_trainable_stage=2)
    f = resnet.plan(50, 6, 256, 704)
    L = p['layers']
    assert len(L) == 54 and p['first_kept'] == 11
    # clear + amax + seed, per trainable convolution weight gradient + fold (42 of them), per block two data gradients (13 blocks) and one to the
    # block's input for every block but layer2.0
    assert p['launches'] == 3 + 2 * 42 + 2 * 13 + 12 == 125
    assert p['forward_workspace_bytes'] == f['workspace_bytes'] and p['forward_pack_bytes'] == f['pack_bytes']
    assert [l['trainable'] for l in L] == [0] * 12 + [1] * 42
    assert [i for i, l in enumerate(L) if l['trainable'] and not l['dgrad']] == [12, 14]          # layer2.0's conv1 and downsample
    assert [l['kept'] for l in L[:12]] == [-1] * 11 + [-2]                                        # layer1's output is outs[0]
    assert [i for i, l in enumerate(L) if l['kept'] <= -2] == [11, 24, 43, 53] and [L[i]['kept'] for i in (24, 43, 53)] == [-3, -4, -5]
    # slabs: 6 x 64 x 176 = 67584 pixels in front of layer2's stride, 16896 behind it, 4224 in layer3, 1056 in layer4
    assert (L[12]['slabs'], L[12]['slab_len']) == (16, 4352)
    assert {(l['slabs'], l['slab_len']) for l in L[13:25]} == {(14, 1280)}
    assert (L[25]['slabs'], L[25]['slab_len']) == (14, 1280) and {(l['slabs'], l['slab_len']) for l in L[26:44]} == {(9, 512)}
    assert (L[44]['slabs'], L[44]['slab_len']) == (9, 512) and {(l['slabs'], l['slab_len']) for l in L[45:]} == {(3, 512)}
    # kept activations: every launch from layer2.0.conv1 on that is not a stage map, 256-byte aligned, in launch order
    rows = lambda i: 6 * f['layers'][i]['h'] * f['layers'][i]['w'] * f['layers'][i]['cout'] * 2
    at = 0
    for i in range(12, 54):
        if L[i]['kept'] >= 0:
            assert L[i]['kept'] == at
            at += (rows(i) + 255) // 256 * 256
    assert p['acts_bytes'] == at == 223838208
    # the backward's pack: per block conv3, conv2, conv1, downsample; layer2.0 packs conv3 and conv2 only
    assert (L[15]['pack_offset'], L[13]['pack_offset']) == (0, 512 * 128 * 2) and L[12]['pack_offset'] == L[14]['pack_offset'] == -1
    b = [L[i]['pack_offset'] for i in (28, 26, 25, 27)]
    assert b[1] - b[0] == 1024 * 256 * 2 and b[2] - b[1] == 9 * 256 * 256 * 2 and b[3] - b[2] == 512 * 256 * 2          # layer3.0: ds right behind conv1
    assert p['pack_bytes'] == sum(f['layers'][i]['taps'] * f['layers'][i]['cin'] * f['layers'][i]['cout'] * 2 for i in range(12, 54) if L[i]['dgrad'])
    g3 = 6 * 32 * 88 * 512 * 2
    assert p['g3_offsets'] == (256, 256 + g3) and p['g2_offset'] == 256 + 2 * g3 and p['g1_offset'] == p['g2_offset'] + 6 * 32 * 88 * 128 * 2
    assert p['part_offset'] == p['g1_offset'] + 6 * 64 * 176 * 128 * 2
    assert p['workspace_bytes'] == p['part_offset'] + 4 * max(l['slabs'] * (fl['taps'] * fl['cin'] * fl['cout'] + fl['cout'])
                                                             for l, fl in zip(L, f['layers']) if l['trainable'])
    # all four stages trainable: the pool's output is the first kept activation, layer1.0 sends nothing to it
    q = resnet.backward_plan(50, 6, 256, 704, first_trainable_stage=1)
    assert q['first_kept'] == 1 and q['layers'][1]['kept'] == 0 and [l['trainable'] for l in q['layers']] == [0, 0] + [1] * 52
    assert [i for i, l in enumerate(q['layers']) if l['trainable'] and not l['dgrad']] == [2, 4]
    z = resnet.backward_plan(50, 0, 256, 704)
    assert z['launches'] == 0 and z['workspace_bytes'] == 0 and z['acts_bytes'] == 0
    big = resnet.backward_plan(50, 48, 256, 704)
    assert big['acts_bytes'] == 8 * p['acts_bytes'] and big['launches'] == 125


def test_backward_plan_refusals():
    table = [
        (dict(first_trainable_stage=0), 'a trainable stem'),
        (dict(first_trainable_stage=5), 'first_trainable_stage=5 not in 1 .. num_stages=4'),
        (dict(first_trainable_stage=-1), 'first_trainable_stage=-1'),
        (dict(depth=18), 'BasicBlock'),
        (dict(base_channels=96), 'multiples of 64'),
        (dict(n=-1), 'n=-1'),
        (dict(H=0), 'empty image'),
        (dict(out_indices=(2, 1)), 'increasing'),
        (dict(n=4096, H=8192, W=8192), '32-bit row indices'),
    ]
    for overrides, text in table:
        args = dict(depth=50, n=1, H=64, W=64)
        args.update(overrides)
        with pytest.raises(SbevError, match=text):
            resnet.backward_plan(**args)


def test_c_entries_validate_before_any_gpu_call(lib):
    one, odd, two = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1008), ctypes.c_void_p(0x1002)
    err = lambda: lib.sbev_last_error().decode()
    dgrad = lambda gy=one, gy2=None, pack=one, mask=None, res=None, gp=None, gdt=0, scale=None, gx=one, n=1, H=4, W=4, cin=64, cout=64, taps=1, \
        stride=1, cout2=0, stride2=1, ct=0: lib.sbev_conv_dgrad_f16(gy, gy2, pack, mask, res, gp, gdt, scale, gx, n, H, W, cin, cout, taps, stride,
                                                                    cout2, stride2, ct, None)
    for overrides, text in [(dict(taps=4), 'taps=4'), (dict(stride=3), 'stride=3'), (dict(cin=96), '96 input channels'), (dict(cout=32), '32 output channels'),
                            (dict(cout2=96), 'Cout2=96'), (dict(cout2=64, stride2=3), 'stride2=3'), (dict(gdt=1), 'gp_dtype 1'),
                            (dict(ct=128), 'col_tile=128'), (dict(n=-1), 'n=-1'), (dict(H=0), 'empty plane'), (dict(W=40000), 'a side above 32767'),
                            (dict(n=1 << 20, H=256, W=256), 'row indices are 32-bit'), (dict(gy=None), 'null pointer'), (dict(pack=None), 'null pointer'),
                            (dict(gx=None), 'null pointer'), (dict(cout2=64), 'null pointer'), (dict(gp=one), 'null pointer'),
                            (dict(gy=odd), '16-byte alignment'), (dict(mask=odd), '16-byte alignment'), (dict(res=odd), '16-byte alignment'),
                            (dict(gp=odd, scale=one), '16-byte alignment'), (dict(gp=one, scale=two), '16-byte alignment')]:
        assert dgrad(**overrides) == -1 and text in err(), (overrides, err())
    assert dgrad(n=0, gy=None, pack=None, gx=None) == 0 and dgrad(n=0, cin=96) == -1

    wgrad = lambda gy=one, x=one, part=one, n=1, H=4, W=4, cin=64, cout=64, taps=1, stride=1, sl=0: lib.sbev_conv_wgrad_f16(
        gy, x, part, n, H, W, cin, cout, taps, stride, sl, None)
    for overrides, text in [(dict(taps=3), 'taps=3'), (dict(stride=0), 'stride=0'), (dict(cin=32), '32 input channels'), (dict(sl=48), 'slab_len=48'),
                            (dict(sl=-32), 'slab_len=-32'), (dict(n=70000, H=64, W=64, sl=32), 'slabs (at most 65535)'), (dict(gy=None), 'null pointer'),
                            (dict(part=None), 'null pointer'), (dict(x=odd), '16-byte alignment'), (dict(part=odd), '16-byte alignment')]:
        assert wgrad(**overrides) == -1 and text in err(), (overrides, err())
    assert wgrad(n=0, gy=None, x=None, part=None) == 0

    fold = lambda part=one, slabs=1, scale=None, w=one, dt=0, gamma=one, mean=one, var=one, eps=1e-5, cin=64, cout=64, taps=1, gw=one, gg=None, gb=None: \
        lib.sbev_bn_fold_backward(part, slabs, scale, w, dt, gamma, mean, var, eps, cin, cout, taps, gw, gg, gb, None)
    for overrides, text in [(dict(slabs=0), 'slabs=0'), (dict(dt=1), 'w_dtype 1'), (dict(eps=-1.0), 'eps'), (dict(taps=2), 'taps=2'),
                            (dict(cout=96), '96 output channels'), (dict(part=None), 'null pointer'), (dict(gw=None), 'null pointer'),
                            (dict(mean=None), 'null pointer'), (dict(gg=two), 'misaligned'), (dict(scale=two), 'misaligned'), (dict(w=two), 'misaligned')]:
        assert fold(**overrides) == -1 and text in err(), (overrides, err())

    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)
    ptrs = lambda *v: (ctypes.c_void_p * len(v))(*v)
    w = ptrs(0x1000)
    pack = lambda n=1, desc=i32(64, 64, 1), w=w, g=w, v=w, eps=1e-5, dt=0, dst=one: lib.sbev_resnet_pack_weights_bwd(n, desc, w, g, v, eps, dt, dst, None)
    for overrides, text in [(dict(desc=i32(96, 64, 1)), '96 input channels'), (dict(desc=i32(64, 64, 49)), 'taps=49'), (dict(dt=1), 'w_dtype 1'),
                            (dict(n=161), '161 layers'), (dict(eps=-1.0), 'eps'), (dict(w=None), 'null pointer'), (dict(dst=None), 'null pointer'),
                            (dict(v=ptrs(0)), 'layer 0: null pointer'), (dict(g=ptrs(0x1002)), 'misaligned'), (dict(dst=odd), '16-byte alignment')]:
        assert pack(**overrides) == -1 and text in err(), (overrides, err())
    assert pack(n=0, w=None, dst=None) == 0

    blocks, idx = i32(1, 1, 1, 1), i32(0, 1, 2, 3)
    outs = ptrs(0x1000, 0x1000, 0x1000, 0x1000)
    fwd = lambda fts=2, n=1, x=one, dt=0, pack=one, ws=one, acts=one, outs=outs, H=32: lib.sbev_resnet_forward_train(
        50, blocks, 4, 64, n, H, 32, 4, idx, fts, x, dt, pack, ws, acts, outs, None)
    for overrides, text in [(dict(fts=0), 'a trainable stem'), (dict(fts=5), 'first_trainable_stage=5'), (dict(dt=1), 'x_dtype 1'), (dict(H=0), 'empty image'),
                            (dict(acts=None), 'null pointer'), (dict(x=None), 'null pointer'), (dict(outs=ptrs(0x1000, 0, 0x1000, 0x1000)), 'output 1: null pointer'),
                            (dict(acts=odd), '16-byte alignment'), (dict(ws=odd), '16-byte alignment')]:
        assert fwd(**overrides) == -1 and text in err(), (overrides, err())
    assert fwd(n=0, x=None, pack=None, ws=None, acts=None, outs=None) == 0

    nconv = 2 + 3 * 4 + 4 - 1
    every = ptrs(*([0x1000] * nconv))
    holes = ptrs(*([0x1000] * (nconv - 1) + [0]))
    bent = ptrs(*([0x1000] * (nconv - 1) + [0x1002]))
    bwd = lambda fts=2, n=1, acts=one, outs=outs, gouts=outs, gdt=0, pack=one, ws=one, w=every, wdt=0, gamma=every, mean=every, var=every, eps=1e-5, \
        gw=every, gg=every, gb=every, H=32: lib.sbev_resnet_backward(50, blocks, 4, 64, n, H, 32, 4, idx, fts, acts, outs, gouts, gdt, pack, ws, w, wdt,
                                                                     gamma, mean, var, eps, gw, gg, gb, None)
    for overrides, text in [(dict(fts=0), 'a trainable stem'), (dict(fts=7), 'first_trainable_stage=7'), (dict(gdt=1), 'g_dtype 1'), (dict(wdt=3), 'w_dtype 3'),
                            (dict(eps=float('inf')), 'eps'), (dict(H=0), 'empty image'), (dict(acts=None), 'null pointer'), (dict(ws=None), 'null pointer'),
                            (dict(gg=None), 'null pointer'), (dict(gouts=ptrs(0x1000, 0x1000, 0, 0x1000)), 'output 2: null pointer'),
                            (dict(gw=holes), 'convolution 16: null pointer'), (dict(mean=holes), 'convolution 16: null pointer'),
                            (dict(acts=odd), '16-byte alignment'), (dict(ws=odd), '16-byte alignment'), (dict(pack=odd), '16-byte alignment'),
                            (dict(gouts=ptrs(0x1000, 0x1008, 0x1000, 0x1000)), '16-byte alignment'), (dict(gb=bent), '16-byte alignment'),
                            (dict(var=bent), '16-byte alignment')]:
        assert bwd(**overrides) == -1 and text in err(), (overrides, err())
    assert bwd(n=0, acts=None, outs=None, gouts=None, pack=None, ws=None, w=None, gamma=None, mean=None, var=None, gw=None, gg=None, gb=None) == 0


def test_python_refusals_and_trainable_parameters():
    from sparsebev_amd import ResNetBackbone
    with pytest.raises(ValueError, match='frozen_stages=-1 with trainable=True is not built'):
        ResNetBackbone(trainable=True)
    with pytest.raises(ValueError, match='frozen_stages=-1 with trainable=True is not built'):
        ResNetBackbone(trainable=True, frozen_stages=-1)
    with pytest.raises(ValueError, match='norm_eval=False is not built'):
        ResNetBackbone(trainable=True, frozen_stages=1, norm_eval=False)
    blocks = BC.HOST_BLOCKS
    for frozen in (0, 1, 3, 4):
        net = ResNetBackbone(stage_blocks=blocks, trainable=True, frozen_stages=frozen, norm_cfg=dict(type='BN2d', requires_grad=True), with_cp=True)
        assert sorted(k for k, p in net.named_parameters() if p.requires_grad) == sorted(BC.trainable_names(blocks, frozen + 1))
        assert not net.training
    net = ResNetBackbone(stage_blocks=blocks, trainable=True, frozen_stages=1, norm_cfg=dict(type='BN', requires_grad=False))
    assert sorted(k for k, p in net.named_parameters() if p.requires_grad) == sorted(BC.trainable_names(blocks, 2, norms=False))
    # the default stays inference only whatever frozen_stages says
    net = ResNetBackbone(stage_blocks=blocks, frozen_stages=1)
    assert not net.trainable and not any(p.requires_grad for p in net.parameters())
    assert net._trainable_conv_index(2) == list(range(5, 23)) and net._trainable_conv_index(1) == list(range(1, 23))          # 23 convolutions, 0 the stem
