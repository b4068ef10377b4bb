"""The ResNet backbone's backward: the fp64 restatement of its definition (include/sbev_hip.h: sbev_resnet_backward) over resnet_cases'
helpers, shared by test_resnet_bwd_host.py, test_gpu_resnet_bwd.py and tools/bench_backbone_train.py.  Like the forward's restatement it
uses no convolution of torch's and no autograd: a data gradient is k^2 strided scatters of einsums, a weight gradient k^2 einsums over
shifted slices.  test_resnet_bwd_host.py holds it against torch.autograd in fp64 with the roundings off."""
import math
from collections import namedtuple

import torch

import resnet_cases as RC

WINDOW_LOG2 = 3          # SBEV_RESNET_GRAD_WINDOW_LOG2
HOST_BLOCKS = (1, 2, 2, 1)
HOST_IMAGE = (2, 3, 40, 72)


# ---------------------------------------------------------------- single operations, fp64, NCHW
def dgrad(gy, w, stride, H, W):
    """gradient at the input [n, ci, H, W] of a k x k convolution (pad k // 2) from the gradient gy [n, co, h, w] at its output"""
    k = w.shape[2]
    pad = k // 2
    n, _, h, v = gy.shape
    p = torch.zeros(n, w.shape[1], H + 2 * pad, W + 2 * pad, dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            p[:, :, ky:ky + stride * (h - 1) + 1:stride, kx:kx + stride * (v - 1) + 1:stride] += torch.einsum('nohw,oc->nchw', gy, w[:, :, ky, kx])
    return p[:, :, pad:pad + H, pad:pad + W]


def wgrad(gy, x, k, stride):
    """(gW [co, ci, k, k], gb [co]) of a k x k convolution (pad k // 2) with input x and output gradient gy, unscaled"""
    pad = k // 2
    n, c, H, W = x.shape
    _, o, h, v = gy.shape
    p = torch.zeros(n, c, H + 2 * pad, W + 2 * pad, dtype=torch.float64)
    p[:, :, pad:pad + H, pad:pad + W] = x
    gw = torch.zeros(o, c, k, k, dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            gw[:, :, ky, kx] = torch.einsum('nohw,nchw->oc', gy, p[:, :, ky:ky + stride * (h - 1) + 1:stride, kx:kx + stride * (v - 1) + 1:stride])
    return gw, gy.sum(dim=(0, 2, 3))


def slab_rule(pixels):
    """(slabs, slab_len): slab_len = max(512, ceil(pixels / 16) rounded up to a multiple of 256)"""
    per = -(-pixels // 16)
    slab_len = max(512, -(-per // 256) * 256)
    return -(-pixels // slab_len), slab_len


def scale_exponent(amax):
    """e with 2^e amax in [2^W, 2^(W + 1)), capped at 126; 0 for a zero or non-finite amax"""
    if amax == 0 or not math.isfinite(amax):
        return 0
    return min(WINDOW_LOG2 - (math.frexp(amax)[1] - 1), 126)


def fold_parts(gamma, var, rounded, eps=RC.EPS):
    """(s, rinv) per output channel as fp64 values: the device's individually rounded fp32 operations, or plain fp64"""
    if rounded:
        root = torch.sqrt((var.float() + torch.tensor(eps, dtype=torch.float32)).double()).float()
        return (gamma.float() / root).double(), (torch.tensor(1.0, dtype=torch.float32) / root).double()
    rinv = 1.0 / torch.sqrt(var.double() + float(torch.tensor(eps, dtype=torch.float32)))
    return gamma.double() * rinv, rinv


def fold_backward(gwp, gbp, w, gamma, mean, var, rounded):
    """(g_w, g_gamma, g_beta) from the folded convolution's gradients gW', gb' in fp64"""
    s, rinv = fold_parts(gamma, var, rounded)
    dot = (w.double() * gwp).sum(dim=(1, 2, 3))
    return s[:, None, None, None] * gwp, rinv * (dot - mean.double() * gbp), gbp.clone()


# ---------------------------------------------------------------- the whole backward
def blocks_of(layers):
    """the blocks of a net_layers list, first to last: dicts of launch indices c1, c2, ds (None), c3, x (the block's input), stage, block"""
    out, i = [], 2
    while i < len(layers):
        ds = i + 2 if layers[i + 2]['epilogue'] == 'bias' else None
        c3 = i + 3 if ds is not None else i + 2
        stage, block = (int(v) for v in layers[i]['conv'][5:].split('.')[:2])
        out.append(dict(c1=i, c2=i + 1, ds=ds, c3=c3, x=layers[i]['src'], stage=stage - 1, block=block))
        i = c3 + 1
    return out


def backward(acts, params, blocks, gouts, first_trainable_stage, rounded=True):
    """The definition in fp64.  acts: every launch's output (NCHW, fp64 values: RC.reference's list or the device's own); gouts: {stage:
    gradient of that stage map, NCHW}; returns (grads {state-dict name: fp64 gradient}, stored {launch index: the gradient stored at that
    launch's output, scaled domain}, e).  rounded False: no fp16 rounding, the fp64 fold, e = 0."""
    layers = RC.net_layers(blocks)
    ends = RC.stage_ends(blocks)
    q = (lambda t: RC.r16(t)) if rounded else (lambda t: t)
    e = scale_exponent(max(float(g.double().abs().max()) for g in gouts.values())) if rounded else 0
    up, down = 2.0 ** e, 2.0 ** -e

    def wq(i):
        if rounded:
            return RC.folded(params, layers[i])[0].double()
        return RC.folded(params, layers[i], RC.fold64)[1]

    grads, stored = {}, {}

    def param_grads(i, gy, x):
        L = layers[i]
        gw, gb = wgrad(gy, x.double(), L['k'], L['stride'])
        g_w, g_gamma, g_beta = fold_backward(down * gw, down * gb, params[L['conv'] + '.weight'], params[L['bn'] + '.weight'],
                                             params[L['bn'] + '.running_mean'], params[L['bn'] + '.running_var'], rounded)
        grads[L['conv'] + '.weight'], grads[L['bn'] + '.weight'], grads[L['bn'] + '.bias'] = g_w, g_gamma, g_beta

    last = len(blocks) - 1
    G = up * gouts[last].double() if last in gouts else torch.zeros_like(acts[-1], dtype=torch.float64)
    zero = torch.zeros((), dtype=torch.float64)
    for B in reversed(blocks_of(layers)):
        if B['stage'] < first_trainable_stage - 1:
            break
        c1, c2, ds, c3, x = B['c1'], B['c2'], B['ds'], B['c3'], B['x']
        H, W = acts[x].shape[2], acts[x].shape[3]
        g3 = q(torch.where(acts[c3] > 0, G, zero))
        param_grads(c3, g3, acts[c2])
        g2 = q(torch.where(acts[c2] > 0, dgrad(g3, wq(c3), 1, acts[c2].shape[2], acts[c2].shape[3]), zero))
        param_grads(c2, g2, acts[c1])
        g1 = q(torch.where(acts[c1] > 0, dgrad(g2, wq(c2), layers[c2]['stride'], H, W), zero))
        param_grads(c1, g1, acts[x])
        if ds is not None:
            param_grads(ds, g3, acts[x])
        stored[c3], stored[c2], stored[c1] = g3, g2, g1
        if B['stage'] == first_trainable_stage - 1 and B['block'] == 0:
            break
        G = dgrad(g1, wq(c1), 1, H, W)
        if ds is not None:
            G = G + dgrad(g3, wq(ds), layers[ds]['stride'], H, W)
            if x in ends and ends.index(x) in gouts:
                G = G + up * gouts[ends.index(x)].double()
        else:
            G = G + g3
    return grads, stored, e


def trainable_names(blocks, first_trainable_stage, norms=True):
    """state-dict names of the parameters mmdet trains with frozen_stages = first_trainable_stage - 1 and norm_eval=True"""
    names = []
    for L in RC.net_layers(blocks):
        if L['kind'] != 'conv' or int(L['conv'][5]) < first_trainable_stage:
            continue
        names.append(L['conv'] + '.weight')
        if norms:
            names += [L['bn'] + '.weight', L['bn'] + '.bias']
    return names


# ---------------------------------------------------------------- bounds
def stored_bound(v, A, K):
    """resnet_cases.layer_bound: an fp16 value accumulated in fp32 over K products with absolute sum A"""
    return RC.layer_bound(v, A, K)


def accum_bound(A, K):
    """an fp32 value accumulated over K terms with absolute sum A: the accumulation term of layer_bound alone"""
    return (K + 4) * 2.0 ** -23 * A


# ---------------------------------------------------------------- single-operation cases
DgradCase = namedtuple('DgradCase', ['name', 'n', 'H', 'W', 'cin', 'cout', 'k', 'stride', 'cout2', 'stride2', 'epi', 'catches'])
# epi: letters m (mask), r (residual), p (a stage map's gradient)
DGRAD_CASES = [
    DgradCase('1x1_64_256', 1, 10, 13, 64, 256, 1, 1, 0, 1, 'm', '130 rows across the 128-row tile boundary; mask only'),
    DgradCase('1x1_2048_512', 1, 2, 3, 512, 2048, 1, 1, 0, 1, 'm', 'the late-stage shape: K = 2048 in 32 chunks, six rows'),
    DgradCase('1x1_res', 1, 10, 13, 256, 64, 1, 1, 0, 1, 'mr', 'identity residual added, then masked; 130 rows'),
    DgradCase('1x1_plain', 1, 3, 5, 64, 64, 1, 1, 0, 1, '', 'no epilogue term at all'),
    DgradCase('3x3_1x1', 1, 1, 1, 64, 64, 3, 1, 0, 1, 'm', 'a 1 x 1 plane: eight of nine taps outside'),
    DgradCase('3x3_3x5', 2, 3, 5, 64, 64, 3, 1, 0, 1, 'm', 'every pixel but three per image on a border; the flip'),
    DgradCase('3x3_s2_5x9', 2, 5, 9, 128, 128, 3, 2, 0, 1, 'm', 'stride 2 from an odd plane (3 x 5 gradients): parity classes, a tile over two images'),
    DgradCase('3x3_s2_6x8', 2, 6, 8, 128, 128, 3, 2, 0, 1, 'm', 'stride 2 from an even plane: the last row and column have one tap row / column'),
    DgradCase('1x1_ds_s2_odd', 2, 5, 9, 256, 64, 1, 1, 512, 2, 'mp', 'conv1 + the stride-2 downsample in one K loop on an odd plane, + 2^e gP'),
    DgradCase('1x1_ds_s1', 1, 3, 5, 64, 64, 1, 1, 256, 1, 'mp', 'the second segment at stride 1 (stage 1 shape), fp32 gP'),
]
DGRAD_BY_NAME = {c.name: c for c in DGRAD_CASES}

WgradCase = namedtuple('WgradCase', ['name', 'n', 'H', 'W', 'cin', 'cout', 'k', 'stride', 'slab_len', 'catches'])
WGRAD_CASES = [
    WgradCase('1x1_1px', 1, 1, 1, 64, 64, 1, 1, 0, 'one pixel'),
    WgradCase('3x3_1px', 1, 1, 1, 64, 64, 3, 1, 0, 'one pixel, eight taps outside'),
    WgradCase('1x1_511', 1, 7, 73, 64, 256, 1, 1, 0, 'slab_len - 1 pixels'),
    WgradCase('1x1_512', 1, 8, 64, 256, 64, 1, 1, 0, 'slab_len pixels: one full slab'),
    WgradCase('1x1_513', 1, 19, 27, 64, 64, 1, 1, 0, 'slab_len + 1 pixels: a second slab of one pixel'),
    WgradCase('3x3_slabs', 2, 3, 25, 64, 128, 3, 1, 64, '150 pixels in three slabs of 64 (the last short), taps across image borders'),
    WgradCase('3x3_s2_5x9', 2, 5, 9, 128, 128, 3, 2, 0, 'the input read at stride 2, odd plane'),
    WgradCase('3x3_s2_6x8', 2, 6, 8, 128, 64, 3, 2, 0, 'the input read at stride 2, even plane; a half column tile'),
    WgradCase('1x1_s2_odd', 2, 5, 9, 256, 512, 1, 2, 0, 'the downsample: 1 x 1 at stride 2, several tiles both ways'),
    WgradCase('1x1_wide', 1, 2, 3, 2048, 512, 1, 1, 0, 'the late-stage shape: 16 x 4 tiles'),
]
WGRAD_BY_NAME = {c.name: c for c in WGRAD_CASES}


def integer_gradient(shape, g, nonzeros=3):
    """a few small integer non-zeros per pixel: values in {-2 .. 2} on `nonzeros` random channels of every pixel, NCHW"""
    n, c, h, w = shape
    vals = torch.randint(-2, 3, shape, generator=g).float()
    rank = torch.rand(n, c, h, w, generator=g).argsort(dim=1).argsort(dim=1)
    return vals * (rank < nonzeros)
