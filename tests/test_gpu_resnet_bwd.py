"""The ResNet backbone's backward on the device against the fp64 restatement of its definition (resnet_bwd_cases.py), into NaN-filled
destinations throughout.  Integers make the structural tests exact (torch.equal): one data gradient and one weight gradient of every
kind, the fold backward, the backward pack bit for bit.  Real-valued data is held operation by operation against fp64 on the device's
own kept activations and incoming gradients (so no mask can flip), inside the worst-case fp32 accumulation bounds; a chain of single
operations reproduces sbev_resnet_backward bit for bit, which ties the checked operations to the one call.  Then scaling, autograd,
capture and the chain image front end -> backbone -> neck."""
import functools

import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

import resnet_bwd_cases as BC  # noqa: E402
import resnet_cases as RC  # noqa: E402
from sparsebev_amd import resnet as R  # noqa: E402

DEV = 'cuda:0'
F16, F32, F64 = torch.float16, torch.float32, torch.float64
BLOCKS = BC.HOST_BLOCKS


def nan(shape, dtype=F32):
    return torch.full(shape, float('nan'), dtype=dtype, device=DEV)


def nchw(t):
    """a device [n, H, W, C] tensor as fp64 NCHW values on the CPU"""
    return t.permute(0, 3, 1, 2).cpu().double()


def scale_pair(e):
    return torch.tensor([2.0 ** e, 2.0 ** -e], dtype=F32, device=DEV)


# ---- 1. one data gradient, exact on integers -----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def integer_dgrad(name):
    """integer data and the fp64 restatement, computed once per case and never written to"""
    c = BC.DGRAD_BY_NAME[name]
    g = torch.Generator().manual_seed(31)
    pad = c.k // 2
    h, v = RC.out_side(c.H, c.k, c.stride, pad), RC.out_side(c.W, c.k, c.stride, pad)
    gy = BC.integer_gradient((c.n, c.cout, h, v), g)
    layer = (RC.sparse_integer_weight(c.cout, c.cin, c.k, 32, g),) + RC.integer_norm(c.cout, g)
    wq = RC.fold32(*layer)[0]
    acc = BC.dgrad(gy.double(), wq.double(), c.stride, c.H, c.W)
    gy2 = layer2 = None
    if c.cout2:
        gy2 = BC.integer_gradient((c.n, c.cout2, RC.out_side(c.H, 1, c.stride2, 0), RC.out_side(c.W, 1, c.stride2, 0)), g)
        layer2 = (RC.sparse_integer_weight(c.cout2, c.cin, 1, 32, g),) + RC.integer_norm(c.cout2, g)
        acc = acc + BC.dgrad(gy2.double(), RC.fold32(*layer2)[0].double(), c.stride2, c.H, c.W)
    shape = (c.n, c.cin, c.H, c.W)
    mask = torch.randint(-1, 3, shape, generator=g).float()
    res = torch.randint(-2, 3, shape, generator=g).float()
    gp = torch.randint(-2, 3, shape, generator=g).float()
    want = acc
    if 'r' in c.epi:
        want = want + res.double()
    if 'p' in c.epi:
        want = want + 4.0 * gp.double()
    if 'm' in c.epi:
        want = torch.where(mask > 0, want, torch.zeros((), dtype=F64))
    return gy, layer, gy2, layer2, mask, res, gp, acc, want


@pytest.mark.parametrize('name', [c.name for c in BC.DGRAD_CASES])
def test_dgrad_exact_on_integers(name):
    c = BC.DGRAD_BY_NAME[name]
    gy, layer, gy2, layer2, mask, res, gp, acc, want = integer_dgrad(name)
    # the premises of exactness, on the CPU first: folded integers, a few small integer non-zeros per pixel, every value an fp16 integer
    assert torch.equal(RC.fold32(*layer)[0].float(), RC.fold32(*layer)[0].float().round()) and float(RC.fold32(*layer)[0].float().abs().max()) == 2.0
    assert int((gy != 0).sum(dim=1).max()) <= 3 and float(gy.abs().max()) == 2.0
    assert float(acc.abs().max()) + 2 + 8 < 2 ** 11 and torch.equal(want, want.round()) and float(acc.abs().max()) >= 2
    if 'm' in c.epi:
        assert bool(((mask <= 0) & (acc != 0)).any()) and bool(((mask > 0) & (acc != 0)).any())          # the mask has work to do
    if c.stride == 2:
        assert all(bool((acc[:, :, y::2, x::2] != 0).any()) for y in (0, 1) for x in (0, 1))            # every parity class gets taps
    layers = [tuple(t.to(DEV) for t in (layer[0], layer[1], layer[4]))]
    if layer2 is not None:
        layers.append(tuple(t.to(DEV) for t in (layer2[0], layer2[1], layer2[4])))
    pack, offs = R.pack_layers_bwd(layers)
    assert offs == [0, c.k ** 2 * c.cin * c.cout * 2][:len(layers)]
    gyd = RC.nhwc(gy, DEV)
    gy2d = None if gy2 is None else RC.nhwc(gy2, DEV)
    for gdt in ((F16, F32) if 'p' in c.epi else (F16,)):
        for ct in [0] + [t for t in (64, 128, 256) if c.cin % t == 0]:
            gx = nan((c.n, c.H, c.W, c.cin), F16)
            R.conv_dgrad_f16(gyd, pack, gx, c.k ** 2, c.stride, gy2=gy2d, stride2=c.stride2, mask=RC.nhwc(mask, DEV) if 'm' in c.epi else None,
                             res=RC.nhwc(res, DEV) if 'r' in c.epi else None, gp=RC.nhwc(gp, DEV, gdt) if 'p' in c.epi else None,
                             scale=scale_pair(2) if 'p' in c.epi else None, col_tile=ct)
            assert torch.equal(nchw(gx), want), 'col_tile %d %s' % (ct, gdt)


def test_backward_pack_holds_the_forward_packs_bits_transposed_and_flipped():
    g = torch.Generator().manual_seed(32)
    layers = []
    for cout, cin, k in ((128, 64, 3), (192, 128, 1), (64, 256, 3)):
        layers.append((torch.randn(cout, cin, k, k, generator=g), 0.5 + torch.rand(cout, generator=g), torch.randn(cout, generator=g),
                       torch.randn(cout, generator=g), 0.01 + 4 * torch.rand(cout, generator=g)))
    for dtype in (F32, F16):
        cast = [tuple(t.to(DEV) for t in ((l[0].to(dtype),) + l[1:])) for l in layers]
        fpack, foffs, _ = R.pack_layers(cast, eps=RC.EPS)
        bpack, boffs = R.pack_layers_bwd([(l[0], l[1], l[4]) for l in cast], eps=RC.EPS)
        for l, fo, bo in zip(cast, foffs, boffs):
            cout, cin, k = l[0].shape[:3]
            wq = RC.unpack_fragments(fpack, fo, cout, cin, k)[0]
            assert torch.equal(wq, RC.fold32(*[t.cpu() for t in l])[0])
            image = torch.cat([bpack[bo:bo + k * k * cin * cout * 2], torch.zeros(4 * cin, dtype=torch.uint8, device=DEV)])
            wt = RC.unpack_fragments(image, 0, cin, cout, k)[0]          # the forward's layout with the channel roles swapped
            assert torch.equal(wt, wq.permute(1, 0, 2, 3).flip(2, 3)), (dtype, tuple(l[0].shape))


# ---- 2. one weight gradient and the fold backward, exact on integers -----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def integer_wgrad(name):
    c = BC.WGRAD_BY_NAME[name]
    g = torch.Generator().manual_seed(33)
    pad = c.k // 2
    h, v = RC.out_side(c.H, c.k, c.stride, pad), RC.out_side(c.W, c.k, c.stride, pad)
    gy = BC.integer_gradient((c.n, c.cout, h, v), g)
    x = torch.randint(-2, 3, (c.n, c.cin, c.H, c.W), generator=g).float()
    layer = (RC.sparse_integer_weight(c.cout, c.cin, c.k, 64, g),) + RC.integer_norm(c.cout, g)
    gw, gb = BC.wgrad(gy.double(), x.double(), c.k, c.stride)
    want = BC.fold_backward(gw / 8, gb / 8, layer[0], layer[1], layer[3], layer[4], rounded=True)
    return gy, x, layer, gw, gb, want


@pytest.mark.parametrize('name', [c.name for c in BC.WGRAD_CASES])
def test_wgrad_and_fold_exact_on_integers(name):
    c = BC.WGRAD_BY_NAME[name]
    gy, x, layer, gw, gb, want = integer_wgrad(name)
    pixels = gy.shape[0] * gy.shape[2] * gy.shape[3]
    slabs, slab_len = (-(-pixels // c.slab_len), c.slab_len) if c.slab_len else BC.slab_rule(pixels)
    # premises: integer sums far below 2^24 in every partial, the 2^-3 scale exact, the folded results exact in fp32
    assert float(BC.wgrad(gy.double().abs(), x.double().abs(), c.k, c.stride)[0].max()) < 2 ** 20
    assert float((layer[0].double().abs() * gw.abs()).sum(dim=(1, 2, 3)).max()) < 2 ** 24 and torch.equal(layer[4] + torch.tensor(RC.EPS), torch.ones(c.cout))
    assert all(torch.equal(t, t.float().double()) for t in want)
    if name == '1x1_513':
        assert (slabs, slab_len) == (2, 512) and pixels == 513
    if name in ('1x1_511', '1x1_512'):
        assert slabs == 1 and pixels == slab_len - (name == '1x1_511')
    if name == '3x3_slabs':
        assert slabs == 3 and pixels % slab_len
    stride = c.k ** 2 * c.cout * c.cin + c.cout
    part = nan((slabs, stride))
    R.conv_wgrad_f16(RC.nhwc(gy, DEV), RC.nhwc(x, DEV), part, c.k ** 2, c.stride, c.slab_len)
    assert bool(torch.isfinite(part).all())
    total = part.cpu().double().sum(dim=0)
    assert torch.equal(total[:stride - c.cout].view(c.k ** 2, c.cout, c.cin).permute(1, 2, 0).reshape(gw.shape), gw), 'partials'
    assert torch.equal(total[stride - c.cout:], gb), 'column sums'
    w, gamma, beta, mean, var = (t.to(DEV) for t in layer)
    for wd in (F32, F16):
        g_w, g_gamma, g_beta = nan(tuple(w.shape)), nan((c.cout,)), nan((c.cout,))
        R.bn_fold_backward(part, w.to(wd), gamma, mean, var, RC.EPS, g_w, g_gamma, g_beta, scale=scale_pair(3))
        assert torch.equal(g_w.cpu().double(), want[0]) and torch.equal(g_gamma.cpu().double(), want[1]) and torch.equal(g_beta.cpu().double(), want[2])
    # a frozen norm: null destinations are skipped
    g_w = nan(tuple(w.shape))
    R.bn_fold_backward(part, w, gamma, mean, var, RC.EPS, g_w, None, None, scale=scale_pair(3))
    assert torch.equal(g_w.cpu().double(), want[0])


@pytest.mark.parametrize('cin,k', [(64, 1), (512, 3)], ids=['K64', 'K4608'])
def test_fold_backward_exact_on_integers(cin, k):
    g = torch.Generator().manual_seed(34)
    cout, slabs = 64, 3
    w = RC.sparse_integer_weight(cout, cin, k, 10 ** 9, g)
    gamma, beta, mean, var = RC.integer_norm(cout, g)
    part = torch.randint(-3, 4, (slabs, k * k * cout * cin + cout), generator=g).float()
    gwp = part.double().sum(dim=0)[:k * k * cout * cin].view(k * k, cout, cin).permute(1, 2, 0).reshape(w.shape)
    gbp = part.double().sum(dim=0)[k * k * cout * cin:]
    assert float((w.double().abs() * gwp.abs()).sum(dim=(1, 2, 3)).max()) < 2 ** 24 and bool((w == 0).any())
    want = BC.fold_backward(gwp, gbp, w, gamma, mean, var, rounded=True)
    g_w, g_gamma, g_beta = nan(tuple(w.shape)), nan((cout,)), nan((cout,))
    R.bn_fold_backward(part.to(DEV), w.to(DEV), gamma.to(DEV), mean.to(DEV), var.to(DEV), RC.EPS, g_w, g_gamma, g_beta)
    assert torch.equal(g_w.cpu().double(), want[0]) and torch.equal(g_gamma.cpu().double(), want[1]) and torch.equal(g_beta.cpu().double(), want[2])
    assert float(want[1].abs().max()) > 16


# ---- 3. the whole net on real data ---------------------------------------------------------------------------------------------------

def make_net(frozen_stages, seed=41, out_indices=(0, 1, 2, 3), norms=True):
    from sparsebev_amd import ResNetBackbone
    params = RC.real_params(BLOCKS, seed=seed)
    net = ResNetBackbone(depth=50, stage_blocks=BLOCKS, out_indices=out_indices, trainable=True, frozen_stages=frozen_stages,
                         norm_cfg=dict(type='BN2d', requires_grad=norms))
    net.load_state_dict(params, strict=True)
    return net.to(DEV), params


def image(seed=42):
    return torch.randn(*BC.HOST_IMAGE, generator=torch.Generator().manual_seed(seed)).to(DEV)


def stage_gradients(outs, seed, dtype=F32, scale=1e-2):
    g = torch.Generator().manual_seed(seed)
    return [(scale * torch.randn(tuple(o.permute(0, 2, 3, 1).shape), generator=g)).to(device=DEV, dtype=dtype).permute(0, 3, 1, 2) for o in outs]


def forward_kept(net, x):
    """a trainable forward: (the stage maps, every launch's output as a device [n, h, w, C] tensor or None where it is not kept)"""
    with torch.enable_grad():
        outs = net(x)
    acts = outs[0].grad_fn.acts
    n, H, W = x.shape[0], x.shape[2], x.shape[3]
    bp, fp = net.backward_plan(n, H, W), net.plan(n, H, W)
    kept = []
    for l, f in zip(bp['layers'], fp['layers']):
        shape = (n, f['h'], f['w'], f['cout'])
        if l['kept'] == -1:
            kept.append(None)
        elif l['kept'] <= -2:
            kept.append(outs[-2 - l['kept']].detach().permute(0, 2, 3, 1))
        else:
            kept.append(acts[l['kept']:l['kept'] + 2 * shape[0] * shape[1] * shape[2] * shape[3]].view(F16).view(shape))
    return outs, acts, kept, bp, fp


def backward_by_hand(net, x, acts, outs, gouts):
    """sbev_resnet_backward into NaN-filled destinations: ({state-dict name: gradient}, the workspace)"""
    n, H, W = x.shape[0], x.shape[2], x.shape[3]
    pairs = net.conv_bn_pairs()
    index = net._trainable_conv_index(net.frozen_stages + 1)
    gw, gg, gb = ([None] * len(pairs) for _ in range(3))
    for j in index:
        gw[j], gg[j], gb[j] = nan(tuple(pairs[j][0].weight.shape)), nan(tuple(pairs[j][1].weight.shape)), nan(tuple(pairs[j][1].bias.shape))
    ws = torch.zeros(net.backward_plan(n, H, W)['workspace_bytes'], dtype=torch.uint8, device=DEV)
    assert all(t.permute(0, 2, 3, 1).is_contiguous() for t in list(outs) + list(gouts))          # the raw call reads channels-last memory
    R.backward_raw(net, n, H, W, net.frozen_stages + 1, acts, [o.detach() for o in outs], gouts, net.pack_bwd(), ws, gw, gg, gb)
    names = [k for k, _ in net.named_parameters()]
    by_id = {id(p): k for k, p in net.named_parameters()}
    grads = {}
    for j in index:
        grads[by_id[id(pairs[j][0].weight)]], grads[by_id[id(pairs[j][1].weight)]], grads[by_id[id(pairs[j][1].bias)]] = gw[j], gg[j], gb[j]
    assert set(grads) <= set(names)
    return grads, ws


@functools.lru_cache(maxsize=None)
def real_case(frozen_stages, gdtype):
    """one forward + one by-hand backward of the issue's net, shared by the tests below and never written to"""
    net, params = make_net(frozen_stages)
    x = image()
    outs, acts, kept, bp, fp = forward_kept(net, x)
    gouts = stage_gradients(outs, 43, gdtype)
    grads, ws = backward_by_hand(net, x, acts, outs, gouts)
    torch.cuda.synchronize()
    return net, params, x, outs, acts, kept, bp, fp, gouts, grads, ws


def chain_of_single_operations(net, kept, bp, gouts, scale):
    """The backward as the header lists it, one single-operation entry per launch, every buffer kept: ({launch: stored gradient
    [n, h, w, C]}, {launch: (g_w, g_gamma, g_beta)}, {launch of a block input: its stored g3})"""
    layers = RC.net_layers(BLOCKS)
    pairs = net.conv_bn_pairs()
    fts = net.frozen_stages + 1
    pack = net.pack_bwd()
    stored, grads = {}, {}

    def params(i, gy, xin):
        L, (conv, bn) = layers[i], pairs[i - 1]
        slabs, slab_len = bp['layers'][i]['slabs'], bp['layers'][i]['slab_len']
        part = nan((slabs, L['k'] ** 2 * L['cout'] * L['cin'] + L['cout']))
        R.conv_wgrad_f16(gy, xin, part, L['k'] ** 2, L['stride'])
        out = nan(tuple(conv.weight.shape)), nan((L['cout'],)), nan((L['cout'],))
        R.bn_fold_backward(part, conv.weight, bn.weight, bn.running_mean, bn.running_var, net.eps, *out, scale=scale)
        grads[i] = out

    last = len(layers) - 1
    ends = RC.stage_ends(BLOCKS)
    gp_of = {e: gouts[net.out_indices.index(s)].permute(0, 2, 3, 1) for s, e in enumerate(ends) if s in net.out_indices}
    g3 = torch.zeros_like(kept[last])
    if last in gp_of:
        g3 = torch.where(kept[last] > 0, (gp_of[last].float() * scale[0]).half(), g3)
    for B in reversed(BC.blocks_of(layers)):
        if B['stage'] < fts - 1:
            break
        c1, c2, ds, c3, x = B['c1'], B['c2'], B['ds'], B['c3'], B['x']
        image_at = lambda i: pack[bp['layers'][i]['pack_offset']:]
        stored[c3] = g3
        params(c3, g3, kept[c2])
        g2 = R.conv_dgrad_f16(g3, image_at(c3), nan(tuple(kept[c2].shape), F16), 1, 1, mask=kept[c2])
        params(c2, g2, kept[c1])
        g1 = R.conv_dgrad_f16(g2, image_at(c2), nan(tuple(kept[c1].shape), F16), 9, layers[c2]['stride'], mask=kept[c1])
        params(c1, g1, kept[x])
        if ds is not None:
            params(ds, g3, kept[x])
        stored[c2], stored[c1] = g2, g1
        if B['stage'] == fts - 1 and B['block'] == 0:
            break
        gp = gp_of.get(x) if ds is not None else None
        g3 = R.conv_dgrad_f16(g1, image_at(c1), nan(tuple(kept[x].shape), F16), 1, 1, gy2=g3 if ds is not None else None,
                              stride2=layers[ds]['stride'] if ds is not None else 1, mask=kept[x], res=None if ds is not None else g3,
                              gp=gp, scale=scale)
    return stored, grads


def operation_errors(frozen_stages):
    """Every stored fp16 gradient inside 2^-11 |v| + 2^-25 + (K + 4) 2^-23 A (resnet_cases.layer_bound: K = the products of one element,
    A = their absolute sum in fp64, the residual and 2^e gP inside A); every fp32 parameter gradient inside the accumulation term alone,
    (K + 4) 2^-23 A with K = the pixels of the reduction + the slabs (g_gamma: + the taps x Cin terms of its dot product, A = rinv
    (sum |w| A_w + |mean| A_b): the weight-gradient errors enter through the dot product, whose own fp32 sum adds taps x Cin roundings).
    The fp64 side runs on the DEVICE's own kept activations and stored gradients."""
    net, params, x, outs, acts, kept, bp, fp, gouts, grads, ws = real_case(frozen_stages, F32)
    scale = ws[:8].view(F32)
    e = BC.scale_exponent(max(float(g.abs().max()) for g in gouts))
    assert scale.tolist() == [2.0 ** e, 2.0 ** -e] and e > 0
    stored, chain = chain_of_single_operations(net, kept, bp, gouts, scale)
    layers = RC.net_layers(BLOCKS)
    names = BC.trainable_names(BLOCKS, frozen_stages + 1)
    assert sorted(grads) == sorted(names)
    # the chain IS the one call: bit-equal parameter gradients
    for i, (g_w, g_gamma, g_beta) in chain.items():
        L = layers[i]
        assert torch.equal(g_w, grads[L['conv'] + '.weight']) and torch.equal(g_gamma, grads[L['bn'] + '.weight']), L['conv']
        assert torch.equal(g_beta, grads[L['bn'] + '.bias']), L['conv']
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())

    up, down = 2.0 ** e, 2.0 ** -e
    ends = RC.stage_ends(BLOCKS)
    K = {i: nchw(k) if k is not None else None for i, k in enumerate(kept)}
    S = {i: nchw(s) for i, s in stored.items()}
    wq = {i: RC.folded(params, layers[i])[0].double() for i in stored}
    ratios, amax = {}, {}

    def note(family, ratio):
        ratios[family] = max(ratios.get(family, 0.0), float(ratio))

    def check_stored(family, got, s, A, k, mask):
        zero = torch.zeros((), dtype=F64)
        s, A = torch.where(mask > 0, s, zero), torch.where(mask > 0, A, zero)
        note(family, ((got - s).abs() / BC.stored_bound(s, A, k)).max())

    last = len(layers) - 1
    assert torch.equal(S[last], RC.r16(torch.where(K[last] > 0, up * nchw(gouts[3].permute(0, 2, 3, 1)), torch.zeros((), dtype=F64)))), 'seed'
    for B in reversed(BC.blocks_of(layers)):
        if B['stage'] < frozen_stages:
            break
        c1, c2, ds, c3, xi = B['c1'], B['c2'], B['ds'], B['c3'], B['x']
        H, W = K[xi].shape[2], K[xi].shape[3]
        for i in (c3, c2, c1):
            amax[i] = float(S[i].abs().max())
        check_stored('dgrad_1x1', S[c2], BC.dgrad(S[c3], wq[c3], 1, *K[c2].shape[2:]), BC.dgrad(S[c3].abs(), wq[c3].abs(), 1, *K[c2].shape[2:]),
                     layers[c3]['cout'], K[c2])
        st = layers[c2]['stride']
        check_stored('dgrad_3x3_s%d' % st, S[c1], BC.dgrad(S[c2], wq[c2], st, H, W), BC.dgrad(S[c2].abs(), wq[c2].abs(), st, H, W),
                     9 * layers[c2]['cout'], K[c1])
        for i, gy, xin in ((c3, S[c3], K[c2]), (c2, S[c2], K[c1]), (c1, S[c1], K[xi])) + (((ds, S[c3], K[xi]),) if ds is not None else ()):
            L = layers[i]
            gw, gb = BC.wgrad(gy, xin, L['k'], L['stride'])
            Aw, Ab = BC.wgrad(gy.abs(), xin.abs(), L['k'], L['stride'])
            w, gamma, mean, var = (params[L['conv'] + '.weight'], params[L['bn'] + '.weight'], params[L['bn'] + '.running_mean'],
                                   params[L['bn'] + '.running_var'])
            want = BC.fold_backward(down * gw, down * gb, w, gamma, mean, var, rounded=True)
            s, rinv = BC.fold_parts(gamma, var, True)
            terms = gy.shape[0] * gy.shape[2] * gy.shape[3] + bp['layers'][i]['slabs']
            fam = 'wgrad_%dx%d_s%d' % (L['k'], L['k'], L['stride'])
            got = [grads[L['conv'] + '.weight'].cpu().double(), grads[L['bn'] + '.weight'].cpu().double(), grads[L['bn'] + '.bias'].cpu().double()]
            tiny = 2.0 ** -126
            note(fam, ((got[0] - want[0]).abs() / (BC.accum_bound(s.abs()[:, None, None, None] * down * Aw, terms) + tiny)).max())
            note('beta', ((got[2] - want[2]).abs() / (BC.accum_bound(down * Ab, terms) + tiny)).max())
            A_gamma = rinv * ((w.double().abs() * down * Aw).sum(dim=(1, 2, 3)) + mean.double().abs() * down * Ab)
            note('gamma', ((got[1] - want[1]).abs() / (BC.accum_bound(A_gamma, terms + L['k'] ** 2 * L['cin']) + tiny)).max())
        if B['stage'] == frozen_stages and B['block'] == 0:
            break
        s, A = BC.dgrad(S[c1], wq_of(params, layers, c1), 1, H, W), BC.dgrad(S[c1].abs(), wq_of(params, layers, c1).abs(), 1, H, W)
        k = layers[c1]['cout']
        if ds is not None:
            wd = wq_of(params, layers, ds)
            s, A = s + BC.dgrad(S[c3], wd, layers[ds]['stride'], H, W), A + BC.dgrad(S[c3].abs(), wd.abs(), layers[ds]['stride'], H, W)
            k += layers[ds]['cout']
            if xi in ends:
                gp = up * nchw(gouts[ends.index(xi)].permute(0, 2, 3, 1))
                s, A = s + gp, A + gp.abs()
        else:
            s, A = s + S[c3], A + S[c3].abs()
        check_stored('dgrad_to_block_input' + ('_downsample' if ds is not None else ''), S[xi], s, A, k, K[xi])
    return ratios, amax


@pytest.mark.parametrize('frozen_stages', [1, 0])
def test_real_data_operation_by_operation(frozen_stages):
    """operation_errors' bounds hold: every stored fp16 gradient and every fp32 parameter gradient of the net, on the device's own inputs"""
    ratios, amax = operation_errors(frozen_stages)
    print('resnet backward frozen_stages=%d: largest error / bound per family %s; scaled-domain amax across the depth: largest %.3g, smallest %.3g'
          % (frozen_stages, {k: round(v, 4) for k, v in sorted(ratios.items())}, max(amax.values()), min(amax.values())))
    assert all(v <= 1.0 for v in ratios.values()), ratios
    assert max(amax.values()) < 65504 and min(amax.values()) > 0


def wq_of(params, layers, i):
    return RC.folded(params, layers[i])[0].double()


def test_restatement_follows_the_device_end_to_end():
    """the rounded fp64 restatement on the device's activations: masks equal, so the two differ by accumulated roundings only -- every
    parameter gradient within 2 % of its tensor's largest entry (a loose whole-net sanity check beside the per-operation bounds)"""
    net, params, x, outs, acts, kept, bp, fp, gouts, grads, ws = real_case(1, F32)
    A = [nchw(k) if k is not None else None for k in kept]
    want, _, e = BC.backward(A, params, BLOCKS, {s: nchw(g.permute(0, 2, 3, 1)) for s, g in enumerate(gouts)}, 2)
    assert ws[:8].view(F32).tolist() == [2.0 ** e, 2.0 ** -e]
    for name, g in grads.items():
        assert float((g.cpu().double() - want[name]).abs().max()) <= 2e-2 * float(want[name].abs().max()), name


# ---- 4. scaling ----------------------------------------------------------------------------------------------------------------------

def test_power_of_two_scaling_zeros_and_inf():
    net, params, x, outs, acts, kept, bp, fp, gouts, grads, ws = real_case(1, F32)
    for p in (-20, 10):
        scaled, ws2 = backward_by_hand(net, x, acts, outs, [g * 2.0 ** p for g in gouts])
        assert ws2[:8].view(F32).tolist() == [v * 2.0 ** (-p if i == 0 else p) for i, v in enumerate(ws[:8].view(F32).tolist())]
        for name, g in grads.items():
            assert torch.equal(scaled[name], g * 2.0 ** p), (p, name)
    zeros, ws0 = backward_by_hand(net, x, acts, outs, [torch.zeros_like(g) for g in gouts])
    assert ws0[:8].view(F32).tolist() == [1.0, 1.0] and all(not bool(g.any()) for g in zeros.values())
    bad = [g.clone() for g in gouts]
    where = (outs[3].detach() > 0).nonzero()[0]
    bad[3][tuple(where)] = float('inf')
    inf, wsi = backward_by_hand(net, x, acts, outs, bad)
    assert wsi[:8].view(F32).tolist() == [1.0, 1.0]
    assert not bool(torch.isfinite(inf['layer4.0.bn3.bias'][where[1]])) and not bool(torch.isfinite(inf['layer4.0.conv3.weight'][where[1]]).all())
    assert not bool(torch.isfinite(inf['layer2.0.conv2.weight']).all())


def test_fp16_gradients_and_fewer_outputs():
    """fp16 output gradients give what their fp32 copies give; out_indices (1, 3) seeds from stage 4 and adds stage 2's gradient only"""
    net, params, x, outs, acts, kept, bp, fp, gouts, grads, ws = real_case(1, F32)
    g16 = [g.permute(0, 2, 3, 1).half().permute(0, 3, 1, 2) for g in gouts]
    a, _ = backward_by_hand(net, x, acts, outs, g16)
    b, _ = backward_by_hand(net, x, acts, outs, [g.float() for g in g16])
    assert all(torch.equal(a[k], b[k]) for k in a)
    net2, _ = make_net(1, out_indices=(1, 3))
    outs2, acts2, kept2, bp2, _ = forward_kept(net2, x)
    assert torch.equal(outs2[0], outs[1]) and torch.equal(outs2[1], outs[3])
    got, _ = backward_by_hand(net2, x, acts2, outs2, [gouts[1], gouts[3]])
    A = [nchw(k) if k is not None else None for k in kept2]
    want, _, _ = BC.backward(A, params, BLOCKS, {1: nchw(gouts[1].permute(0, 2, 3, 1)), 3: nchw(gouts[3].permute(0, 2, 3, 1))}, 2)
    for name in ('layer2.0.conv2.weight', 'layer3.1.bn2.weight', 'layer4.0.downsample.0.weight'):
        assert float((got[name].cpu().double() - want[name]).abs().max()) <= 2e-2 * float(want[name].abs().max()), name
        # stage 4 hears from its own map only (the same as with four outputs); stages 2 and 3 miss stage 3's addend
        assert torch.equal(got[name], grads[name]) == name.startswith('layer4'), name


# ---- 5. autograd ---------------------------------------------------------------------------------------------------------------------

def loss_of(outs, gouts):
    """a loss whose gradient at the fp16 maps is gouts (fp16 values) exactly"""
    return sum((o.float() * g.float()).sum() for o, g in zip(outs, gouts))


def test_module_gradients_equal_the_c_entry_and_repeat_bit_for_bit():
    net, params, x, outs, acts, kept, bp, fp, gouts, grads, ws = real_case(1, F16)
    mod, _ = make_net(1)
    runs = []
    for _ in range(2):
        mod.zero_grad(set_to_none=True)
        with torch.enable_grad():
            o = mod(x)
            assert all(torch.equal(a, b) for a, b in zip(o, outs)) and all(t.requires_grad and t.dtype == F16 for t in o)
            assert all(t.permute(0, 2, 3, 1).is_contiguous() for t in o)
            loss_of(o, gouts).backward()
        runs.append({k: p.grad.clone() for k, p in mod.named_parameters() if p.grad is not None})
    assert sorted(runs[0]) == sorted(grads) == sorted(BC.trainable_names(BLOCKS, 2))
    for k, g in grads.items():
        assert runs[0][k].dtype == F32 and torch.equal(runs[0][k], g) and torch.equal(runs[1][k], g), k
    assert all(p.grad is None for k, p in mod.named_parameters() if k not in grads)
    # .grad accumulates over a second backward, and an NCHW-contiguous or fp16 output gradient is taken (one copy)
    with torch.enable_grad():
        o = mod(x)
        torch.autograd.backward(o, [g.contiguous() for g in gouts])
    for k, g in grads.items():
        assert torch.equal(dict(mod.named_parameters())[k].grad, g + g), k


def test_two_forwards_in_flight_and_frozen_norms():
    net, params, x, outs, acts, kept, bp, fp, gouts, grads, ws = real_case(1, F16)
    mod, _ = make_net(1, norms=False)
    x2 = image(44)
    with torch.enable_grad():
        o1 = mod(x)
        o2 = mod(x2)                      # a second node with a buffer of its own before the first one's backward
        assert o1[0].grad_fn.acts.data_ptr() != o2[0].grad_fn.acts.data_ptr()
        loss_of(o2, gouts).backward()
        second = {k: p.grad.clone() for k, p in mod.named_parameters() if p.grad is not None}
        mod.zero_grad(set_to_none=True)
        loss_of(o1, gouts).backward()
    names = BC.trainable_names(BLOCKS, 2, norms=False)
    assert sorted(second) == sorted(names) and all('bn' not in k and 'downsample.1' not in k for k in names)
    for k in names:
        assert torch.equal(dict(mod.named_parameters())[k].grad, grads[k]), k          # the first forward's activations survived the second
        assert not torch.equal(second[k], grads[k])
    with torch.enable_grad():
        with pytest.raises(ValueError, match='no image gradient is ever produced'):
            mod(x.clone().requires_grad_(True))
        with pytest.raises(ValueError, match='out= / keep= are not taken'):
            mod(x, keep=[])
        mod.conv1.weight.requires_grad_(True)
        with pytest.raises(RuntimeError, match='conv1.weight requires a gradient but lies in the frozen part'):
            mod(x)


def test_no_grad_equals_the_inference_module_and_an_optimizer_step_repacks():
    from sparsebev_amd import ResNetBackbone
    from sparsebev_amd.optim import FusedAdamW
    net, params, x, outs, acts, kept, bp, fp, gouts, grads, ws = real_case(1, F16)
    mod, _ = make_net(1)
    plain = ResNetBackbone(depth=50, stage_blocks=BLOCKS)
    plain.load_state_dict(params, strict=True)
    plain = plain.to(DEV)
    with torch.no_grad():
        a, b = mod(x), plain(x)
    assert all(torch.equal(p, q) and not p.requires_grad for p, q in zip(a, b)) and all(torch.equal(p, q) for p, q in zip(a, outs))
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match='inference only'):
            plain.layer4[0].conv1.weight.requires_grad_(True)
            plain(x)
    opt = FusedAdamW([p for p in mod.parameters() if p.requires_grad], lr=1e-2)
    with torch.enable_grad():
        loss_of(mod(x), gouts).backward()
    keys = (mod._image.key, mod._image_bwd.key)
    before = mod.pack_bwd().clone()
    at = mod.pack().data_ptr(), mod.pack_bwd().data_ptr()
    opt.step()
    with torch.enable_grad():
        o = mod(x)
    assert mod._image.key != keys[0] and mod._image_bwd.key != keys[1] and not torch.equal(mod.pack_bwd(), before)
    assert (mod.pack().data_ptr(), mod.pack_bwd().data_ptr()) == at          # both repacked in place
    assert torch.equal(o[0], outs[0]) and not torch.equal(o[1], outs[1])          # stage 1 is frozen, stage 2 moved
    # the next forward and backward see the new weights: a fresh module on the stepped parameters agrees bit for bit
    fresh, _ = make_net(1)
    fresh.load_state_dict(mod.state_dict(), strict=True)
    mod.zero_grad(set_to_none=True)
    with torch.enable_grad():
        loss_of(o, gouts).backward()
        loss_of(fresh(x), gouts).backward()
    for (k, p), (_, q) in zip(mod.named_parameters(), fresh.named_parameters()):
        assert (p.grad is None and q.grad is None) or torch.equal(p.grad, q.grad), k


def test_trainable_forward_refused_under_capture():
    mod, _ = make_net(1)
    x = image()
    with torch.enable_grad():
        mod(x)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.enable_grad(), pytest.raises(RuntimeError, match='a trainable forward under a graph capture'):
        with torch.cuda.graph(graph):
            mod(x)


# ---- 6. capture of the C backward ----------------------------------------------------------------------------------------------------

def test_captured_backward_replays_on_overwritten_gradients():
    net, params, x, outs, acts, kept, bp, fp, gouts, grads, ws = real_case(1, F32)
    n, H, W = x.shape[0], x.shape[2], x.shape[3]
    pairs = net.conv_bn_pairs()
    index = net._trainable_conv_index(2)
    gw, gg, gb = ([None] * len(pairs) for _ in range(3))
    for j in index:
        gw[j], gg[j], gb[j] = nan(tuple(pairs[j][0].weight.shape)), nan(tuple(pairs[j][1].weight.shape)), nan(tuple(pairs[j][1].bias.shape))
    static = [torch.zeros_like(g) for g in gouts]
    wsc = torch.zeros_like(ws)
    pack = net.pack_bwd()
    detached = [o.detach() for o in outs]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        R.backward_raw(net, n, H, W, 2, acts, detached, static, pack, wsc, gw, gg, gb)          # warm-up on zeros
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            R.backward_raw(net, n, H, W, 2, acts, detached, static, pack, wsc, gw, gg, gb)
    torch.cuda.current_stream().wait_stream(stream)
    by_id = {id(p): k for k, p in net.named_parameters()}
    for factor in (1.0, 2.0 ** -7):          # the second replay has another amax: the scale is found inside the graph
        for s, g in zip(static, gouts):
            s.copy_(g * factor)
        for t in gw + gg + gb:
            if t is not None:
                t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        for j in index:
            assert torch.equal(gw[j], grads[by_id[id(pairs[j][0].weight)]] * factor), (factor, j)
            assert torch.equal(gg[j], grads[by_id[id(pairs[j][1].weight)]] * factor) and torch.equal(gb[j], grads[by_id[id(pairs[j][1].bias)]] * factor)
    assert wsc[:8].view(F32).tolist() == [v * (2.0 ** 7 if i == 0 else 2.0 ** -7) for i, v in enumerate(ws[:8].view(F32).tolist())]


# ---- 7. image front end -> backbone -> neck ------------------------------------------------------------------------------------------

def test_front_end_backbone_neck_end_to_end():
    from sparsebev_amd import FPNNeck, ImageFrontEnd
    mod, _ = make_net(1)
    torch.manual_seed(45)
    neck = FPNNeck([256, 512, 1024, 2048], 256, 4, trainable=True).to(DEV)
    front = ImageFrontEnd(dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True), out_dtype=F16).to(DEV).eval()
    img = torch.randint(0, 256, BC.HOST_IMAGE, generator=torch.Generator().manual_seed(46), dtype=torch.uint8).to(DEV)
    with torch.no_grad():
        x = front(img, [dict()])
    g = torch.Generator().manual_seed(47)
    with torch.enable_grad():
        stages = mod(x)
        for s in stages:
            s.retain_grad()
        pyramid = neck(stages, out_dtype=F32)
        weights = [torch.randn(tuple(p.shape), generator=g).to(DEV) for p in pyramid]
        sum((p * w).sum() for p, w in zip(pyramid, weights)).backward()
    handed = [s.grad for s in stages]
    assert [(None if h is None else (h.dtype, tuple(h.shape))) for h in handed] == [(F16, tuple(s.shape)) for s in stages]
    # what autograd retains may be a copy in another layout; the node takes either (one copy), the raw call reads channels-last memory
    handed = [h if h.permute(0, 2, 3, 1).is_contiguous() else h.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) for h in handed]
    want, _ = backward_by_hand(mod, x, stages[0].grad_fn.acts, stages, handed)
    got = {k: p.grad for k, p in mod.named_parameters() if p.grad is not None}
    assert sorted(got) == sorted(want) == sorted(BC.trainable_names(BLOCKS, 2))
    for k in want:
        assert torch.equal(got[k], want[k]) and bool(torch.isfinite(got[k]).all()) and bool(got[k].any()), k
    assert all(p.grad is not None for p in neck.parameters())
