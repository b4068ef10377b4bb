"""The ResNet backbone's cases and the fp64 restatement of its definition (include/sbev_hip.h: sbev_resnet_forward), shared by
test_resnet_host.py, test_gpu_resnet.py and tools/bench_backbone.py.  The restatement uses no convolution and no pooling of torch's: a
k x k convolution is k^2 strided, shifted einsums over a zero-padded plane, the max-pool nine shifted slices of a plane padded with -inf.
test_resnet_host.py holds it against F.conv2d / F.batch_norm / F.max_pool2d with the roundings off."""
from collections import namedtuple

import torch

ConvCase = namedtuple('ConvCase', ['name', 'n', 'H', 'W', 'cin', 'cout', 'k', 'stride', 'catches'])

CONV_CASES = [
    ConvCase('1x1_rows130', 1, 10, 13, 64, 64, 1, 1, '130 rows: the 128-row boundary falls mid-row; the narrow column tile'),
    ConvCase('1x1_s2_odd', 2, 5, 9, 256, 512, 1, 2, 'an odd plane 5 x 9 -> 3 x 5, a tile that spans images, column tiles of 64, 128 and 256'),
    ConvCase('3x3_1x1', 1, 1, 1, 64, 64, 3, 1, 'a 1 x 1 plane: eight of nine taps outside'),
    ConvCase('3x3_3x5', 2, 3, 5, 64, 64, 3, 1, 'every pixel but three per image on a border'),
    ConvCase('3x3_s2_5x9', 2, 5, 9, 128, 128, 3, 2, 'stride 2 on an odd plane: the last row and column read (2 y + 1, 2 x + 1) outside'),
    ConvCase('3x3_s2_4x8', 2, 4, 8, 128, 128, 3, 2, 'stride 2 on an even plane: tap (2, 2) of the last pixel is the last source pixel'),
    ConvCase('1x1_wide', 1, 2, 3, 512, 2048, 1, 1, 'many column tiles, six rows: the late-stage shape'),
]
CONV_BY_NAME = {c.name: c for c in CONV_CASES}
EPILOGUES = ('bias', 'relu', 'residual_relu')
EPS = 1e-5


def col_tiles(cout):
    """every column tile width sbev_conv_f16 accepts for this Cout, and 0 (the plan's choice)"""
    return [0] + [ct for ct in (64, 128, 256) if cout % ct == 0]


def out_side(size, k, stride, pad):
    return (size + 2 * pad - k) // stride + 1


# ---------------------------------------------------------------- the restatement, fp64
def r16(t, on=True):
    """round to fp16 (nearest even) and back to fp64"""
    return t.half().double() if on else t.double()


def conv(x, w, stride, pad):
    """k x k convolution of x [n, c, H, W] with w [o, c, k, k], zero padding, fp64 in, fp64 out"""
    n, c, H, W = x.shape
    k = w.shape[2]
    h, v = out_side(H, k, stride, pad), out_side(W, k, stride, pad)
    p = torch.zeros(n, c, H + 2 * pad, W + 2 * pad, dtype=x.dtype)
    p[:, :, pad:pad + H, pad:pad + W] = x
    out = torch.zeros(n, w.shape[0], h, v, dtype=x.dtype)
    for ky in range(k):
        for kx in range(k):
            out += torch.einsum('nchw,oc->nohw', p[:, :, ky:ky + stride * (h - 1) + 1:stride, kx:kx + stride * (v - 1) + 1:stride], w[:, :, ky, kx])
    return out


def max_pool(x):
    """3 x 3 / 2 / pad 1 ignoring the padding"""
    n, c, H, W = x.shape
    h, v = out_side(H, 3, 2, 1), out_side(W, 3, 2, 1)
    p = torch.full((n, c, H + 2, W + 2), float('-inf'), dtype=x.dtype)
    p[:, :, 1:H + 1, 1:W + 1] = x
    out = torch.full((n, c, h, v), float('-inf'), dtype=x.dtype)
    for ky in range(3):
        for kx in range(3):
            out = torch.maximum(out, p[:, :, ky:ky + 2 * (h - 1) + 1:2, kx:kx + 2 * (v - 1) + 1:2])
    return out


def scale32(gamma, var, eps=EPS):
    """s = gamma / sqrt(var + eps), three correctly rounded fp32 operations.  The square root is taken in fp64 and rounded to fp32: that
    IS the correctly rounded fp32 root (53 >= 2 x 24 + 2 bits: the double rounding is innocuous), while torch's own fp32 CPU sqrt is
    not always (it differs from IEEE on about 6 of 1000 arguments)."""
    root = torch.sqrt((var.float() + torch.tensor(eps, dtype=torch.float32)).double()).float()
    return gamma.float() / root


def fold32(w, gamma, beta, mean, var, eps=EPS):
    """The fold as the device does it, in fp32 operations each rounded on its own: (w' fp16, b' fp32)"""
    s = scale32(gamma, var, eps)
    return (w.float() * s[:, None, None, None]).half(), beta.float() - mean.float() * s


def fold64(w, gamma, beta, mean, var, eps=EPS):
    """The fold in fp64 from the same fp32 values (eps as the fp32 number the device adds): (s, w s, b)"""
    eps = float(torch.tensor(eps, dtype=torch.float32))
    s = gamma.double() / torch.sqrt(var.double() + eps)
    return s, w.double() * s[:, None, None, None], beta.double() - mean.double() * s


def conv_layer(x, wq, bq, stride, pad, epilogue, residual=None):
    """(s, A) of one folded convolution BEFORE its rounding, in fp64: x the fp16-valued input activation, wq / bq the folded weight and
    bias; A = sum of absolute products + |b'| (+ |residual|) bounds the accumulation error"""
    x, wq, bq = x.double(), wq.double(), bq.double()
    s = conv(x, wq, stride, pad) + bq[None, :, None, None]
    A = conv(x.abs(), wq.abs(), stride, pad) + bq.abs()[None, :, None, None]
    if epilogue == 'residual_relu':
        s, A = s + residual.double(), A + residual.double().abs()
    if epilogue != 'bias':
        s = s.clamp_min(0.0)
    return s, A


def layer_bound(s, A, K):
    """tests/fpn_cases.py::stage_errors' worst-case bound of an fp16 result accumulated in fp32 over K products"""
    return 2.0 ** -11 * s.abs() + 2.0 ** -25 + (K + 4) * 2.0 ** -23 * A


# ---------------------------------------------------------------- the net as a list of launches
def net_layers(blocks, base=64):
    """The launches of a backbone in launch order (the C entry's: stem, pool, per block conv1, conv2, [downsample], conv3) as dicts:
    kind, name (the state-dict prefix of the convolution and of its norm), cin, cout, k, stride, pad, epilogue, src / res (indices of
    the launches whose outputs it reads; -1: the image)"""
    L = [dict(kind='stem', conv='conv1', bn='bn1', cin=3, cout=base, k=7, stride=2, pad=3, epilogue='relu', src=-1, res=None),
         dict(kind='pool', src=0, cout=base)]
    cur, cin = 1, base
    for s, nb in enumerate(blocks):
        mid = base << s
        for b in range(nb):
            st = 2 if (b == 0 and s > 0) else 1
            pre = 'layer%d.%d.' % (s + 1, b)
            L.append(dict(kind='conv', conv=pre + 'conv1', bn=pre + 'bn1', cin=cin, cout=mid, k=1, stride=1, pad=0, epilogue='relu', src=cur, res=None))
            L.append(dict(kind='conv', conv=pre + 'conv2', bn=pre + 'bn2', cin=mid, cout=mid, k=3, stride=st, pad=1, epilogue='relu', src=len(L) - 1,
                          res=None))
            t2, res = len(L) - 1, cur
            if b == 0:
                L.append(dict(kind='conv', conv=pre + 'downsample.0', bn=pre + 'downsample.1', cin=cin, cout=4 * mid, k=1, stride=st, pad=0,
                              epilogue='bias', src=cur, res=None))
                res = len(L) - 1
            L.append(dict(kind='conv', conv=pre + 'conv3', bn=pre + 'bn3', cin=mid, cout=4 * mid, k=1, stride=1, pad=0, epilogue='residual_relu',
                          src=t2, res=res))
            cur, cin = len(L) - 1, 4 * mid
    return L


def stage_ends(blocks):
    """index of the launch that writes each stage's output"""
    layers = net_layers(blocks)
    ends, at = [], 1
    for s, nb in enumerate(blocks):
        at += 3 * nb + 1
        ends.append(at)
    assert all(layers[e]['epilogue'] == 'residual_relu' for e in ends)
    return ends


def folded(params, layer, fold=fold32):
    c, b = layer['conv'], layer['bn']
    return fold(params[c + '.weight'], params[b + '.weight'], params[b + '.bias'], params[b + '.running_mean'], params[b + '.running_var'])


def reference(x, params, blocks, rounded=True):
    """The whole net in fp64, NCHW: the output of every launch.  ``rounded`` False switches every fp16 rounding off and applies the
    norm with the fp64 fold."""
    acts = []
    for layer in net_layers(blocks):
        src = r16(x, rounded) if layer['src'] < 0 else acts[layer['src']]
        if layer['kind'] == 'pool':
            acts.append(max_pool(src))
            continue
        if rounded:
            wq, bq = folded(params, layer)
        else:
            _, wq, bq = folded(params, layer, fold64)
        s, _ = conv_layer(src, wq, bq, layer['stride'], layer['pad'], layer['epilogue'], None if layer['res'] is None else acts[layer['res']])
        acts.append(r16(s, rounded))
    return acts


# ---------------------------------------------------------------- data
def state_dict_shapes(blocks, base=64):
    """name -> shape of every state-dict entry, in launch order"""
    shapes = {}
    for layer in net_layers(blocks, base):
        if layer['kind'] == 'pool':
            continue
        shapes[layer['conv'] + '.weight'] = (layer['cout'], layer['cin'], layer['k'], layer['k'])
        for leaf in ('weight', 'bias', 'running_mean', 'running_var'):
            shapes[layer['bn'] + '.' + leaf] = (layer['cout'],)
        shapes[layer['bn'] + '.num_batches_tracked'] = ()
    return shapes


def real_params(blocks, seed, base=64):
    """He-scaled weights, random positive running_var and gamma (small for bn3: the residual branch stays the smaller term), mean, beta"""
    g = torch.Generator().manual_seed(seed)
    params = {}
    for layer in net_layers(blocks, base):
        if layer['kind'] == 'pool':
            continue
        c, b, co = layer['conv'], layer['bn'], layer['cout']
        params[c + '.weight'] = torch.randn(co, layer['cin'], layer['k'], layer['k'], generator=g) * (2.0 / (layer['cin'] * layer['k'] ** 2)) ** 0.5
        small = b.endswith('bn3')
        params[b + '.weight'] = (0.1 if small else 0.5) + (0.2 if small else 1.0) * torch.rand(co, generator=g)
        params[b + '.bias'] = 0.1 * torch.randn(co, generator=g)
        params[b + '.running_mean'] = 0.1 * torch.randn(co, generator=g)
        params[b + '.running_var'] = 0.5 + torch.rand(co, generator=g)
        params[b + '.num_batches_tracked'] = torch.tensor(0)
    return params


def integer_norm(cout, g):
    """BatchNorm tensors that fold to integers: fp32(var + eps) == 1, gamma in {1, 2}, integer mean and beta"""
    var = torch.full((cout,), 1.0) - torch.tensor(EPS, dtype=torch.float32)
    return (torch.randint(1, 3, (cout,), generator=g).float(), torch.randint(-3, 4, (cout,), generator=g).float(),
            torch.randint(-2, 3, (cout,), generator=g).float(), var)


def sparse_integer_weight(cout, cin, k, keep, g):
    """weights in {-1, 0, 1} with at most ``keep`` non-zeros per output channel"""
    w = torch.randint(-1, 2, (cout, cin * k * k), generator=g).float()
    if cin * k * k > keep:
        rank = torch.rand(cout, cin * k * k, generator=g).argsort(dim=1).argsort(dim=1)
        w = w * (rank < keep)
    return w.view(cout, cin, k, k)


def integer_conv_data(case, seed, keep=64):
    """Small integers on which every product and partial sum is exact: x and residual in {-2 .. 2}, weights in {-1, 0, 1} with at most
    ``keep`` non-zeros per output, a norm that folds to integers.  Returns (x NCHW, residual NCHW, (w, gamma, beta, mean, var))."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, (case.n, case.cin, case.H, case.W), generator=g).float()
    h, v = out_side(case.H, case.k, case.stride, case.k // 2), out_side(case.W, case.k, case.stride, case.k // 2)
    res = torch.randint(-2, 3, (case.n, case.cout, h, v), generator=g).float()
    w = sparse_integer_weight(case.cout, case.cin, case.k, keep, g)
    return x, res, (w,) + integer_norm(case.cout, g)


def integer_params(blocks, seed, base=64, keep=64):
    """a whole net's state dict on integer_conv_data's recipe"""
    g = torch.Generator().manual_seed(seed)
    params = {}
    for layer in net_layers(blocks, base):
        if layer['kind'] == 'pool':
            continue
        c, b = layer['conv'], layer['bn']
        params[c + '.weight'] = sparse_integer_weight(layer['cout'], layer['cin'], layer['k'], keep, g)
        gamma, beta, mean, var = integer_norm(layer['cout'], g)
        params.update({b + '.weight': gamma, b + '.bias': beta, b + '.running_mean': mean, b + '.running_var': var,
                       b + '.num_batches_tracked': torch.tensor(0)})
    return params


# ---------------------------------------------------------------- device helpers (GPU tests and the bench tool)
def nhwc(x, device, dtype=torch.float16):
    """NCHW values as a contiguous [n, H, W, C] device tensor"""
    return x.to(device=device, dtype=dtype).permute(0, 2, 3, 1).contiguous()


def unpack_fragments(pack, offset, cout, cin, k):
    """One layer's fragment-order image inside a pack tensor back as (w' [cout, cin, k, k] fp16, b' [cout] fp32), on the CPU: lane l of
    fragment nt of k-step ks of tap t holds channel 64 (nt / 2) + 2 (l & 31) + (nt & 1), k index 16 ks + 8 (l >> 5) + j.  The stem
    (k = 7) is one tap over K = 147 (c, ky, kx) padded to 160; the padding must be zero."""
    taps, K = (1, 160) if k == 7 else (k * k, cin)
    real = cin * 49 if k == 7 else cin
    halves = taps * K * cout
    raw = pack[offset:offset + 2 * halves].cpu().view(torch.float16).view(taps, K // 16, cout // 32, 64, 8)
    bias = pack[offset + 2 * halves:offset + 2 * halves + 4 * cout].cpu().view(torch.float32)
    nt, lane, j, ks = torch.arange(cout // 32), torch.arange(64), torch.arange(8), torch.arange(K // 16)
    co = (64 * (nt // 2) + (nt % 2))[:, None] + 2 * (lane % 32)[None, :]                       # [NF, 64]
    kk = 16 * ks[:, None, None] + 8 * (lane // 32)[None, :, None] + j[None, None, :]            # [KS, 64, 8]
    w = torch.zeros(taps, cout, K, dtype=torch.float16)
    w[:, co[None, :, :, None].expand(K // 16, -1, -1, 8), kk[:, None, :, :].expand(-1, cout // 32, -1, -1)] = raw
    assert not w[:, :, real:].any()
    if k == 7:
        return w[0, :, :real].view(cout, cin, 7, 7), bias
    return w.permute(1, 2, 0).reshape(cout, cin, k, k), bias


def layer_errors(keep, x, params, blocks, device='cpu'):
    """Hold every launch's output (``keep`` from ResNetBackbone.forward) against fp64 on the DEVICE's own input activations.  Returns a
    list of dicts, one per launch: name, kind ('stem', 'pool', '1x1', '3x3', 'downsample', 'conv3'), max error, the largest ratio
    error / bound (<= 1 passes; layer_bound with K = taps x Cin, the residual inside A), finite."""
    acts = [k.cpu() for k in keep]
    rows = []
    for i, layer in enumerate(net_layers(blocks)):
        src = x.cpu().half() if layer['src'] < 0 else acts[layer['src']]
        if layer['kind'] == 'pool':
            same = torch.equal(acts[i].double(), max_pool(src.double()))
            rows.append(dict(name='pool', kind='pool', max=0.0 if same else float('inf'), ratio=0.0 if same else float('inf'), finite=True))
            continue
        wq, bq = folded(params, layer)
        s, A = conv_layer(src, wq, bq, layer['stride'], layer['pad'], layer['epilogue'], None if layer['res'] is None else acts[layer['res']])
        err = (acts[i].double() - s).abs()
        kind = ('stem' if layer['kind'] == 'stem' else 'downsample' if layer['epilogue'] == 'bias' else 'conv3' if layer['res'] is not None
                else '%dx%d' % (layer['k'], layer['k']))
        rows.append(dict(name=layer['conv'], kind=kind, max=float(err.max()), ratio=float((err / layer_bound(s, A, layer['cin'] * layer['k'] ** 2)).max()),
                         finite=bool(torch.isfinite(acts[i]).all())))
    return rows


def make_backbone(blocks, params, device, depth=50, out_indices=None):
    from sparsebev_amd import ResNetBackbone
    out_indices = tuple(range(len(blocks))) if out_indices is None else out_indices
    net = ResNetBackbone(depth=depth, num_stages=len(blocks), out_indices=out_indices, stage_blocks=blocks)
    net.load_state_dict(params, strict=True)
    return net.to(device)


def nan_outputs(shapes, device):
    """NaN-filled channels-last destinations for [(n, C, h, w), ...]"""
    return [torch.full((n, h, w, c), float('nan'), dtype=torch.float16, device=device).permute(0, 3, 1, 2) for n, c, h, w in shapes]
