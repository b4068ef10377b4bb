"""The FPN neck's cases and the fp64 restatement of its definition (include/sbev_hip.h: sbev_fpn_forward), shared by test_fpn_host.py,
test_gpu_fpn.py and tools/bench_fpn.py.  The restatement uses no convolution and no interpolation of torch's: a 1 x 1 convolution is an
einsum, a 3 x 3 one nine shifted einsums over a zero-padded plane, the upsampling two index tables (sparsebev_amd.fpn.nearest_index),
an extra level a strided slice.  test_fpn_host.py holds it against F.conv2d / F.interpolate / F.max_pool2d with the roundings off."""
from collections import namedtuple

import torch

from sparsebev_amd.fpn import nearest_index

Case = namedtuple('Case', ['name', 'n', 'planes', 'cin', 'num_outs', 'catches'])

CASES = [
    Case('tiny', 2, [(4, 6), (2, 3), (1, 2), (1, 1)], [32, 64, 96, 128], 4,
         'a pixel tile that spans images, every pixel on a border, a 1 x 1 plane, four workgroups of one partial tile each'),
    Case('odd', 1, [(7, 9), (4, 5), (2, 3), (1, 2)], [32, 64, 32, 64], 4, 'ceil-halves: the nearest rule at ratios other than 2'),
    Case('edges', 2, [(5, 13), (3, 7), (2, 4), (1, 2)], [32, 32, 32, 32], 4,
         'level 0 has 65 pixels per image, 130 in all: the 64- and 128-row tile boundaries fall mid-row and mid-image'),
    Case('r50k', 1, [(8, 8), (4, 4), (2, 2), (1, 1)], [256, 512, 1024, 2048], 4, 'the real K-loop lengths of the r50 stages'),
    Case('five', 1, [(24, 40), (12, 20), (6, 10), (3, 5)], [32, 32, 32, 32], 5,
         'num_outs = 5 with an odd last plane: 3 x 5 gives an extra level of 2 x 3; 960 pixels: seven full tiles and a partial one'),
]
BY_NAME = {c.name: c for c in CASES}


def out_planes(case):
    hw = list(case.planes)
    while len(hw) < case.num_outs:
        hw.append(((hw[-1][0] + 1) // 2, (hw[-1][1] + 1) // 2))
    return hw


# ---------------------------------------------------------------- data
def real_data(case, seed):
    """fp32 inputs (NCHW values) and parameters: unit-scale inputs, weights of the scale Xavier gives, non-zero biases"""
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(case.n, c, h, w, generator=g) for c, (h, w) in zip(case.cin, case.planes)]
    params = {}
    for i, c in enumerate(case.cin):
        params['lateral_convs.%d.conv.weight' % i] = torch.randn(256, c, 1, 1, generator=g) * (2.0 / (c + 256)) ** 0.5
        params['lateral_convs.%d.conv.bias' % i] = torch.randn(256, generator=g) * 0.1
        params['fpn_convs.%d.conv.weight' % i] = torch.randn(256, 256, 3, 3, generator=g) * (2.0 / (9 * 512)) ** 0.5
        params['fpn_convs.%d.conv.bias' % i] = torch.randn(256, generator=g) * 0.1
    return xs, params


def integer_data(case, seed, keep=64):
    """Small integers on which every product and every partial sum is exact in fp16 x fp16 -> fp32: inputs in {-2 .. 2} with at most
    ``keep`` non-zero channels per pixel, weights in {-1, 0, 1}, biases in {-3 .. 3}."""
    g = torch.Generator().manual_seed(seed)
    xs = []
    for c, (h, w) in zip(case.cin, case.planes):
        x = torch.randint(-2, 3, (case.n, c, h, w), generator=g).float()
        if c > keep:
            rank = torch.rand(case.n, c, h, w, generator=g).argsort(dim=1).argsort(dim=1)
            x = x * (rank < keep)
        xs.append(x)
    params = {}
    for i, c in enumerate(case.cin):
        params['lateral_convs.%d.conv.weight' % i] = torch.randint(-1, 2, (256, c, 1, 1), generator=g).float()
        params['lateral_convs.%d.conv.bias' % i] = torch.randint(-3, 4, (256,), generator=g).float()
        params['fpn_convs.%d.conv.weight' % i] = torch.randint(-1, 2, (256, 256, 3, 3), generator=g).float()
        params['fpn_convs.%d.conv.bias' % i] = torch.randint(-3, 4, (256,), generator=g).float()
    return xs, params


# ---------------------------------------------------------------- the restatement, fp64
def r16(t, on=True):
    """round to fp16 (nearest even) and back to fp64"""
    return t.half().double() if on else t.double()


def conv1x1(x, w):
    return torch.einsum('nchw,oc->nohw', x, w[:, :, 0, 0])


def conv3x3(x, w):
    n, c, H, W = x.shape
    p = torch.zeros(n, c, H + 2, W + 2, dtype=x.dtype)
    p[:, :, 1:H + 1, 1:W + 1] = x
    out = torch.zeros(n, w.shape[0], H, W, dtype=x.dtype)
    for ky in range(3):
        for kx in range(3):
            out += torch.einsum('nchw,oc->nohw', p[:, :, ky:ky + H, kx:kx + W], w[:, :, ky, kx])
    return out


def upsample(parent, H, W):
    iy = torch.from_numpy(nearest_index(parent.shape[2], H))
    ix = torch.from_numpy(nearest_index(parent.shape[3], W))
    return parent[:, :, iy][:, :, :, ix]


def lateral_stage(x, w, b, parent, rounded=True):
    """(s, A): the merged lateral BEFORE its rounding, in fp64, from fp16-rounded operands and the given parent (already fp16 values or
    None), and the sum of absolute products + |bias| + |parent| that bounds the accumulation error"""
    x, w, b = r16(x.cpu(), rounded), r16(w.cpu(), rounded), b.cpu().double()
    s = conv1x1(x, w) + b[None, :, None, None]
    A = conv1x1(x.abs(), w.abs()) + b.abs()[None, :, None, None]
    if parent is not None:
        up = upsample(parent.cpu().double(), x.shape[2], x.shape[3])
        s, A = s + up, A + up.abs()
    return s, A


def output_stage(m, w, b, rounded=True):
    """(s, A) of an output convolution over the merged lateral m (fp16 values), as lateral_stage"""
    m, w, b = m.cpu().double(), r16(w.cpu(), rounded), b.cpu().double()
    return conv3x3(m, w) + b[None, :, None, None], conv3x3(m.abs(), w.abs()) + b.abs()[None, :, None, None]


def reference(xs, params, num_outs, rounded=True):
    """The whole neck in fp64: (merged laterals M_l, outputs P_o), NCHW.  ``rounded`` False switches every fp16 rounding off."""
    L = len(xs)
    M = [None] * L
    for l in range(L - 1, -1, -1):
        s, _ = lateral_stage(xs[l], params['lateral_convs.%d.conv.weight' % l], params['lateral_convs.%d.conv.bias' % l],
                             M[l + 1] if l + 1 < L else None, rounded)
        M[l] = r16(s, rounded)
    P = [output_stage(M[l], params['fpn_convs.%d.conv.weight' % l], params['fpn_convs.%d.conv.bias' % l], rounded)[0] for l in range(L)]
    while len(P) < num_outs:
        P.append(P[-1][:, :, ::2, ::2])
    return M, P


# ---------------------------------------------------------------- device helpers (GPU tests and the bench tool)
def channels_last(x):
    """the same [n, C, H, W] values in channels-last memory"""
    return x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def nan_outputs(case, dtype, device):
    """NaN-filled destinations for FPNNeck.forward(out=...)"""
    return [torch.full((case.n, h, w, 256), float('nan'), dtype=dtype, device=device).permute(0, 3, 1, 2) for h, w in out_planes(case)]


def make_neck(case, params, device):
    from sparsebev_amd import FPNNeck
    neck = FPNNeck(case.cin, 256, case.num_outs)
    neck.load_state_dict(params, strict=True)
    return neck.to(device).eval()


def stage_errors(neck, case, xs, params, in_dtype, out_dtype, device):
    """Run the neck and hold every stage against fp64 on the DEVICE's own previous stage.  Returns a list of dicts, one per stage:
    name, max error, rms error, the largest ratio error / bound (<= 1 passes).  Bounds (K = reduction length, A from the stage):
      M_l:            2^-11 |s| + 2^-25 + (K + 4) 2^-23 A
      P_l, fp32 out:  (K + 4) 2^-23 A
      P_l, fp16 out:  2^-11 |s| + 2^-25 + (K + 4) 2^-23 A"""
    dev_in = [channels_last(x.to(device=device, dtype=in_dtype)) for x in xs]
    out = nan_outputs(case, out_dtype, device)
    got = neck(dev_in, out=out)
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    merged = [m.cpu() for m in neck.merged]
    rows = []
    L = len(xs)

    def row(name, g, s, A, K, with_rounding):
        err = (g.double() - s).abs()
        bound = (K + 4) * 2.0 ** -23 * A
        if with_rounding:
            bound = bound + 2.0 ** -11 * s.abs() + 2.0 ** -25
        rows.append(dict(stage=name, max=float(err.max()), rms=float(err.pow(2).mean().sqrt()), ratio=float((err / bound).max()),
                         finite=bool(torch.isfinite(g).all())))

    for l in range(L):
        s, A = lateral_stage(xs[l], params['lateral_convs.%d.conv.weight' % l], params['lateral_convs.%d.conv.bias' % l],
                             merged[l + 1] if l + 1 < L else None)
        row('M%d' % l, merged[l], s, A, case.cin[l], True)
        s, A = output_stage(merged[l], params['fpn_convs.%d.conv.weight' % l], params['fpn_convs.%d.conv.bias' % l])
        row('P%d' % l, got[l].cpu(), s, A, 9 * 256, out_dtype == torch.float16)
    for o in range(L, case.num_outs):
        same = torch.equal(got[o].cpu(), got[o - 1].cpu()[:, :, ::2, ::2])
        rows.append(dict(stage='P%d' % o, max=0.0 if same else float('inf'), rms=0.0 if same else float('inf'), ratio=0.0 if same else float('inf'),
                         finite=bool(torch.isfinite(got[o]).all())))
    return rows
